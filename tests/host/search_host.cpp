// Host build of the search core (csrc/search.hpp: the node step the device
// kernel runs, compiled with g++) for tests/test_search_host.py: as a shared
// library with C linkage, and, with -DSEARCH_MAIN, as a stand-alone program for
// -fsanitize=address,undefined that searches the positions of a text file (one
// position a line: n meta depth mobility terminal value best, then the black,
// white and possible_moves words in hex, then the N*N weights) and compares
// value and best.  Test infrastructure only.
#include <stdint.h>
#include <stdio.h>

#include "../../gymothelloenv_amd/csrc/search.hpp"

using namespace oth;

// boards [E][2W] (black words, then white), meta [E], legal [E][W]: the exchange format
template <int N>
static void search_n(int E, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal, int depth,
                     const int8_t* weights, int mobility, int terminal, uint32_t max_nodes, int32_t* value,
                     int32_t* best, int32_t* move_values, uint8_t* status, uint64_t* nodes) {
    constexpr int W = Geo<N>::W, NN = N * N;
    for (int e = 0; e < E; ++e)
        status[e] = (uint8_t)search_board_host<N>(boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W,
                                                  legal + (size_t)e * W, meta[e], depth, weights, mobility, terminal,
                                                  max_nodes, value + e, best + e, move_values + (size_t)e * NN,
                                                  nodes + e);
}

extern "C" int host_search(int n, int E, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal,
                           int depth, const int8_t* weights, int mobility, int terminal, uint64_t max_nodes,
                           int32_t* value, int32_t* best, int32_t* move_values, uint8_t* status, uint64_t* nodes) {
    if (depth < 1 || depth > SEARCH_MAX_DEPTH || !weights || mobility < -127 || mobility > 127 || terminal < 1 ||
        terminal > 32767 || max_nodes < 1 || max_nodes > 0xffffffffull)
        return -1;
    const uint32_t mn = (uint32_t)max_nodes;
    switch (n) {
#define CASE(K)                                                                                                  \
    case K:                                                                                                      \
        search_n<K>(E, boards, meta, legal, depth, weights, mobility, terminal, mn, value, best, move_values, status, \
                    nodes);                                                                                      \
        break;
#ifdef SEARCH_MAIN  // the sanitizer program's sizes only: one-, two- and four-word frames, a shorter build
        CASE(4) CASE(6) CASE(8) CASE(10) CASE(16)
#else
        CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#endif
#undef CASE
        default: return -1;
    }
    return 0;
}

#ifdef SEARCH_MAIN
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n, meta, depth, mobility, terminal, want_value, want_best, count = 0;
    while (fscanf(f, "%d %d %d %d %d %d %d", &n, &meta, &depth, &mobility, &terminal, &want_value, &want_best) == 7) {
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
        int32_t value, best, mv[256];
        uint8_t status;
        uint64_t nodes;
        if (host_search(n, 1, boards, &m, legal, depth, weights, mobility, terminal, 1u << 24, &value, &best, mv,
                        &status, &nodes))
            return 2;
        if (value != want_value || best != want_best) {
            fprintf(stderr, "FAILED position %d: value %d best %d, expected %d %d\n", count, value, best, want_value,
                    want_best);
            return 1;
        }
        ++count;
    }
    fclose(f);
    if (!count) return 2;
    printf("search core under ASan and UBSan: %d positions clean\n", count);
    return 0;
}
#endif
