// Host build of the network's move (csrc/play_net.hpp's shared part over csrc/net.hpp: the argmax key, the
// draw's word and target, the cumulative scan and one row's move -- the text the device kernel runs, compiled
// with g++) for tests/test_play_net_host.py: a shared library with C linkage.
// tests/host/play_net_san_main.cpp includes this file under -fsanitize=address,undefined.
// Test infrastructure only.
#include <stdint.h>

#include <vector>

#include "../../gymothelloenv_amd/csrc/play_net.hpp"

using namespace oth;

// the plain rule on one row's z, priors, stored legal words, D and u
extern "C" int host_net_move_rule(int nn, const int32_t* z, const int32_t* prior, const uint64_t* stored, int discs,
                                  int sample_discs, uint32_t u) {
    return net_move_row(nn, z, prior, stored, discs, sample_discs, u);
}

extern "C" uint32_t host_net_move_word(uint64_t seed, uint32_t id, uint64_t g) { return net_move_word(seed, id, g); }

// the square a target r picks on a row (the sweep over every r in [0, P))
extern "C" int host_net_sample_square(int nn, const uint64_t* stored, const int32_t* prior, uint32_t r) {
    return net_sample_square(nn, stored, [&](int a) { return prior[a]; }, r);
}

// P of R rows in the exchange format: row r draws with id id_base + r and ply index g[r].  0, 1 for arguments
// out of range, 2 for a blob of another geometry or other shifts (nothing is written)
extern "C" int host_net_moves(int n, const NetParams* p, int R, const uint8_t* blob, const uint64_t* boards,
                              const uint16_t* meta, const uint64_t* legal, int sample_discs, uint64_t seed,
                              uint32_t id_base, const uint64_t* g, int32_t* out) {
    if (net_check(n, p) || sample_discs < 0 || sample_discs > NET_SAMPLE_DISCS_MAX) return 1;
    const NetGeo geo = net_geo(n, *p);
    std::vector<int32_t> priors(geo.nn), z(geo.nn + 1);
    for (int r = 0; r < R; ++r) {
        const uint64_t* bd = boards + (size_t)r * 2 * geo.W;
        const uint64_t* lg = legal + (size_t)r * geo.W;
        int32_t value;
        if (!net_row(geo, blob, bd, meta[r], lg, priors.data(), &value, z.data())) return 2;
        int discs = 0;
        for (int k = 0; k < geo.W; ++k) discs += __builtin_popcountll(bd[k] | bd[geo.W + k]);
        out[r] = net_move_row(geo.nn, z.data(), priors.data(), lg, discs, sample_discs,
                              net_move_word(seed, id_base + (uint32_t)r, g[r]));
    }
    return 0;
}
