// Host build of the play-search core (csrc/play_search.hpp: the depth rule, the
// greedy fallback by solve_flips popcounts, over csrc/search.hpp's node step,
// compiled with g++) for tests/test_play_search_host.py: as a shared library
// with C linkage, and, with -DPLAY_SEARCH_MAIN, as a stand-alone program for
// -fsanitize=address,undefined that moves on the positions of a text file (one
// position a line: n meta depth mobility terminal endgame_empties max_nodes
// action fallback, then the black, white and possible_moves words in hex, then
// the N*N weights) and compares action and fallback.  Test infrastructure only.
#include <stdint.h>
#include <stdio.h>

#include "../../gymothelloenv_amd/csrc/play_search.hpp"

using namespace oth;

// boards [E][2W] (black words, then white), meta [E], legal [E][W]: the exchange format
template <int N>
static void moves_n(int E, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal, const PlaySearchSide& c,
                    int32_t* actions, uint8_t* fallbacks) {
    constexpr int W = Geo<N>::W;
    for (int e = 0; e < E; ++e) {
        int fb;
        actions[e] = play_search_move_host<N>(boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W,
                                              legal + (size_t)e * W, meta[e], c, &fb);
        fallbacks[e] = (uint8_t)fb;
    }
}

extern "C" int host_search_move(int n, int E, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal,
                                int depth, const int8_t* weights, int mobility, int terminal, int endgame_empties,
                                uint64_t max_nodes, int32_t* actions, uint8_t* fallbacks) {
    if (depth < 1 || depth > SEARCH_MAX_DEPTH || !weights || mobility < -127 || mobility > 127 || terminal < 1 ||
        terminal > 32767 || endgame_empties < 0 || endgame_empties > SEARCH_MAX_DEPTH || max_nodes < 1 ||
        max_nodes > 0xffffffffull)
        return -1;
    const PlaySearchSide c{weights, depth, mobility, terminal, endgame_empties, (uint32_t)max_nodes};
    switch (n) {
#define CASE(K)                                                     \
    case K:                                                         \
        moves_n<K>(E, boards, meta, legal, c, actions, fallbacks); \
        break;
#ifdef PLAY_SEARCH_MAIN  // the sanitizer program's sizes only: a shorter build
        CASE(4) CASE(5) CASE(6) CASE(8) CASE(10) CASE(16)
#else
        CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#endif
#undef CASE
        default: return -1;
    }
    return 0;
}

#ifdef PLAY_SEARCH_MAIN
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n, meta, depth, mobility, terminal, endgame, want_action, want_fb, count = 0;
    unsigned long long max_nodes;
    while (fscanf(f, "%d %d %d %d %d %d %llu %d %d", &n, &meta, &depth, &mobility, &terminal, &endgame, &max_nodes,
                  &want_action, &want_fb) == 9) {
        if (n < 4 || n > 16) return 2;
        const int W = (n * n + 63) / 64;
        uint64_t boards[8] = {0}, legal[4] = {0};
        for (int i = 0; i < 3 * W; ++i) {
            unsigned long long x;
            if (fscanf(f, "%llx", &x) != 1) return 2;
            if (i < 2 * W) boards[i] = x;
            else legal[i - 2 * W] = x;
        }
        int8_t weights[256];
        for (int a = 0; a < n * n; ++a) {
            int w;
            if (fscanf(f, "%d", &w) != 1 || w < -128 || w > 127) return 2;
            weights[a] = (int8_t)w;
        }
        const uint16_t m = (uint16_t)meta;
        int32_t action;
        uint8_t fb;
        if (host_search_move(n, 1, boards, &m, legal, depth, weights, mobility, terminal, endgame, max_nodes, &action,
                             &fb))
            return 2;
        if (action != want_action || fb != want_fb) {
            fprintf(stderr, "FAILED position %d: action %d fallback %d, expected %d %d\n", count, action, (int)fb,
                    want_action, want_fb);
            return 1;
        }
        ++count;
    }
    fclose(f);
    if (!count) return 2;
    printf("play-search core under ASan and UBSan: %d positions clean\n", count);
    return 0;
}
#endif
