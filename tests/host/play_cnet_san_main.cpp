// A stand-alone program for -fsanitize=address,undefined over the conv net's move
// (tests/host/play_cnet_host.cpp, included here: the host build of csrc/play_net.hpp's
// shared part over csrc/cnet.hpp), for tests/test_play_cnet_sanitizers.py.  It reads one
// case from stdin, packs the weights into a heap blob of exactly the reported size,
// computes the moves of the rows into arrays of exactly R elements and prints them, a
// line a sample_discs setting.  The input: a line
//   n C B shift_stem shift[0 .. 15] shift_head policy_shift value_shift R seed id_base g0 K
// then the weights, the biases, per row a line (meta, the 3W words in hex), and K values
// of sample_discs; row r draws with id id_base + r and ply index g0 + r.
// Test infrastructure only.
#include <stdio.h>

#include <vector>

#include "play_cnet_host.cpp"

int main() {
    int n, R, K;
    unsigned long long seed, g0;
    unsigned id_base;
    CnetParams p;
    if (scanf("%d %d %d %d", &n, &p.channels, &p.blocks, &p.shift_stem) != 4) return 2;
    for (int l = 0; l < 16; ++l)
        if (scanf("%d", &p.shift[l]) != 1) return 2;
    if (scanf("%d %d %d %d %llu %u %llu %d", &p.shift_head, &p.policy_shift, &p.value_shift, &R, &seed, &id_base, &g0,
              &K) != 8)
        return 2;
    if (cnet_check(n, &p) || R < 1 || K < 1) return 2;
    const CnetGeo geo = cnet_geo(n, p);
    std::vector<int8_t> w(cnet_weights(geo));
    std::vector<int32_t> b(cnet_biases(geo));
    for (size_t i = 0; i < w.size(); ++i) {
        int x;
        if (scanf("%d", &x) != 1) return 2;
        w[i] = (int8_t)x;
    }
    for (size_t i = 0; i < b.size(); ++i)
        if (scanf("%d", &b[i]) != 1) return 2;
    std::vector<uint8_t> blob(geo.bytes(), 0xa5);
    if (cnet_pack(n, p, w.data(), b.data(), blob.data())) return 2;
    const int W = geo.W;
    std::vector<uint64_t> boards((size_t)R * 2 * W), legal((size_t)R * W), g(R);
    std::vector<uint16_t> meta(R);
    for (int r = 0; r < R; ++r) {
        int mt;
        unsigned long long x;
        if (scanf("%d", &mt) != 1) return 2;
        meta[r] = (uint16_t)mt;
        for (int j = 0; j < 3 * W; ++j) {
            if (scanf("%llx", &x) != 1) return 2;
            (j < 2 * W ? boards[(size_t)r * 2 * W + j] : legal[(size_t)r * W + j - 2 * W]) = x;
        }
        g[r] = g0 + (uint64_t)r;
    }
    for (int k = 0; k < K; ++k) {
        int sample_discs;
        if (scanf("%d", &sample_discs) != 1) return 2;
        std::vector<int32_t> moves(R, 7);
        if (host_cnet_moves(n, &p, R, blob.data(), boards.data(), meta.data(), legal.data(), sample_discs, seed, id_base,
                            g.data(), moves.data()))
            return 2;
        printf("%d", sample_discs);
        for (int r = 0; r < R; ++r) printf(" %d", moves[r]);
        printf("\n");
    }
    printf("conv net moves under ASan and UBSan: clean\n");
    return 0;
}
