// Host build of the solver's search core (csrc/solve.hpp: the node step the
// device kernel runs, compiled with g++) for tests/test_solve_host.py: as a
// shared library with C linkage, and, with -DSOLVE_MAIN, as a stand-alone
// program for -fsanitize=address,undefined that solves the positions of a text
// file (one position a line: n meta value best, then the black, white and
// possible_moves words in hex) and compares value and best.  Test infrastructure only.
#include <stdint.h>
#include <stdio.h>

#include "../../gymothelloenv_amd/csrc/solve.hpp"

using namespace oth;

// boards [E][2W] (black words, then white), meta [E], legal [E][W]: the exchange format
template <int N>
static void solve_n(int E, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal, int max_empties,
                    uint32_t max_nodes, int32_t* value, int32_t* best, int32_t* move_values, uint8_t* status,
                    uint64_t* nodes) {
    constexpr int W = Geo<N>::W, NN = N * N;
    for (int e = 0; e < E; ++e)
        status[e] = (uint8_t)solve_board_host<N>(boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W,
                                                 legal + (size_t)e * W, meta[e], max_empties, max_nodes, value + e,
                                                 best + e, move_values + (size_t)e * NN, nodes + e);
}

extern "C" int host_solve(int n, int E, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal,
                          int max_empties, uint64_t max_nodes, int32_t* value, int32_t* best, int32_t* move_values,
                          uint8_t* status, uint64_t* nodes) {
    if (max_empties < 1 || max_empties > SOLVE_MAX_EMPTIES || max_nodes < 1 || max_nodes > 0xffffffffull) return -1;
    const uint32_t mn = (uint32_t)max_nodes;
    switch (n) {
#define CASE(K) \
    case K: solve_n<K>(E, boards, meta, legal, max_empties, mn, value, best, move_values, status, nodes); break;
#ifdef SOLVE_MAIN  // the sanitizer program's sizes only: one-, two- and four-word frames, a shorter build
        CASE(4) CASE(6) CASE(8) CASE(10) CASE(16)
#else
        CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#endif
#undef CASE
        default: return -1;
    }
    return 0;
}

// update_board's flips from the two sides' discs (solve_flips1) for every empty square of one-word boards
template <int N>
static void flips_n(int E, const uint64_t* mover, const uint64_t* opp, uint64_t* out) {
    for (int e = 0; e < E; ++e)
        for (int a = 0; a < N * N; ++a) {
            const bool empty = !(((mover[e] | opp[e]) >> a) & 1ull);
            out[(size_t)e * N * N + a] = empty ? solve_flips1<N>(mover[e], opp[e], a) : 0ull;
        }
}

extern "C" int host_solve_flips_all(int n, int E, const uint64_t* mover, const uint64_t* opp, uint64_t* out) {
    switch (n) {
        case 4: flips_n<4>(E, mover, opp, out); break;
        case 5: flips_n<5>(E, mover, opp, out); break;
        case 6: flips_n<6>(E, mover, opp, out); break;
        case 7: flips_n<7>(E, mover, opp, out); break;
        case 8: flips_n<8>(E, mover, opp, out); break;
        default: return -1;
    }
    return 0;
}

#ifdef SOLVE_MAIN
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n, meta, want_value, want_best, count = 0;
    while (fscanf(f, "%d %d %d %d", &n, &meta, &want_value, &want_best) == 4) {
        const int W = (n * n + 63) / 64;
        uint64_t boards[8] = {0}, legal[4] = {0};
        for (int i = 0; i < 3 * W; ++i) {
            unsigned long long x;
            if (fscanf(f, "%llx", &x) != 1) return 2;
            if (i < 2 * W) boards[i] = x;
            else legal[i - 2 * W] = x;
        }
        const uint16_t m = (uint16_t)meta;
        int32_t value, best, mv[256];
        uint8_t status;
        uint64_t nodes;
        if (host_solve(n, 1, boards, &m, legal, SOLVE_MAX_EMPTIES, 1u << 24, &value, &best, mv, &status, &nodes)) return 2;
        if (value != want_value || best != want_best) {
            fprintf(stderr, "FAILED position %d: value %d best %d, expected %d %d\n", count, value, best, want_value,
                    want_best);
            return 1;
        }
        ++count;
    }
    fclose(f);
    if (!count) return 2;
    printf("solve core under ASan and UBSan: %d positions clean\n", count);
    return 0;
}
#endif
