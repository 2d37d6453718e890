// Host build of the play-ntuple core (csrc/play_ntuple.hpp: the exploring draw, the move T of one
// board over csrc/ntuple.hpp's node step, the greedy fallback and the TD target rule, compiled with
// g++) for tests/test_play_ntuple_host.py: a shared library with C linkage.
// tests/host/play_ntuple_san_main.cpp includes this file under -fsanitize=address,undefined.
// Test infrastructure only.
#include <stddef.h>
#include <stdint.h>

#include "../../gymothelloenv_amd/csrc/play_ntuple.hpp"

using namespace oth;

namespace {

// boards [E][2W] (black words, then white), meta [E], legal [E][W]: the exchange format; ids and g per board
template <int N>
void moves_n(int E, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal, const PlayNtupleSide& c,
             uint64_t seed, const uint32_t* ids, const uint64_t* g, int32_t* actions, uint8_t* fallbacks,
             uint8_t* explored, int32_t* targets) {
    constexpr int W = Geo<N>::W;
    for (int e = 0; e < E; ++e) {
        int fb, ex;
        actions[e] = play_ntuple_move_host<N>(boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W,
                                              legal + (size_t)e * W, meta[e], c, seed, ids[e], g[e], &fb, &ex,
                                              targets ? targets + e : nullptr);
        fallbacks[e] = (uint8_t)fb;
        explored[e] = (uint8_t)ex;
    }
}

}  // namespace

// T of E boards and, where the move is a finished search's, its row's target (else 0; targets may be NULL).
// 0, or -1 for arguments out of range (nothing is written).
extern "C" int host_ntuple_move(int n, int E, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal,
                                const NtupleParams* p, const int32_t* weights, int depth, int terminal,
                                int endgame_empties, int explore, uint64_t max_nodes, uint64_t seed, const uint32_t* ids,
                                const uint64_t* g, int32_t* actions, uint8_t* fallbacks, uint8_t* explored,
                                int32_t* targets) {
    uint32_t plan[NTUPLE_PLAN_WORDS];
    if (!p || ntuple_check(n, p) || !weights || depth < 1 || depth > SEARCH_MAX_DEPTH || terminal < 1 ||
        terminal > 32767 || endgame_empties < 0 || endgame_empties > SEARCH_MAX_DEPTH || explore < 0 ||
        explore > NTUPLE_EXPLORE_ONE || max_nodes < 1 || max_nodes > 0xffffffffull)
        return -1;
    ntuple_plan(n, *p, plan);
    const PlayNtupleSide c{plan, weights, depth, terminal, endgame_empties, explore, (uint32_t)max_nodes};
    switch (n) {
#define CASE(K)                                                                                              \
    case K:                                                                                                  \
        moves_n<K>(E, boards, meta, legal, c, seed, ids, g, actions, fallbacks, explored, targets);          \
        break;
#ifdef PLAY_NTUPLE_SAN_MAIN  // the sanitizer program's sizes only: one-, two- and four-word boards, a shorter build
        CASE(4) CASE(8) CASE(10) CASE(16)
#else
        CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#endif
#undef CASE
        default: return -1;
    }
    return 0;
}
