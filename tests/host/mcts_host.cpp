// Host build of the tree search's core (csrc/mcts.hpp: the descent, the key,
// the backup and the outputs the device kernel runs, with playouts by the
// generic rules, compiled with g++) for tests/test_mcts_host.py: as a shared
// library with C linkage, and, with -DMCTS_MAIN, as a stand-alone program for
// -fsanitize=address,undefined that searches the boards of a text file (a
// header line: n E I R C T seed id_key id_base counter; then one board a line:
// meta status best tree_nodes, the black, white and possible_moves words in
// hex, then N*N visits and N*N wins2) and compares every output.  Test
// infrastructure only.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../gymothelloenv_amd/csrc/mcts.hpp"

using namespace oth;

// boards [E][2W] (black words, then white), meta [E], legal [E][W]: the exchange format
template <int N>
static void mcts_n(int E, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal, uint32_t id_base,
                   const MctsParams& p, int32_t* visits, int32_t* wins2, int32_t* best, int32_t* tree_nodes,
                   uint8_t* status) {
    constexpr int W = Geo<N>::W, NN = N * N;
    std::vector<uint64_t> tree((size_t)p.T * MctsTree<N>::WORDS, 0xdeadbeefdeadbeefull);  // uninitialised, as far as it goes
    for (int e = 0; e < E; ++e)
        status[e] = (uint8_t)mcts_host<N>(boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W,
                                          legal + (size_t)e * W, meta[e], id_base + (uint32_t)e, p, tree.data(),
                                          visits + (size_t)e * NN, wins2 + (size_t)e * NN, best + e, tree_nodes + e);
}

extern "C" int host_mcts(int n, int E, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal,
                         uint32_t id_base, int iterations, int playouts, int c_explore, int max_tree_nodes,
                         uint64_t seed, uint32_t id_key, uint64_t counter, int32_t* visits, int32_t* wins2,
                         int32_t* best, int32_t* tree_nodes, uint8_t* status) {
    if (iterations < 1 || iterations > MCTS_MAX_ITERATIONS || playouts < 1 || playouts > MCTS_MAX_PLAYOUTS ||
        c_explore < 0 || c_explore > MCTS_MAX_C || max_tree_nodes < n * n || max_tree_nodes > MCTS_MAX_TREE_NODES ||
        counter >> 56)
        return -1;
    const MctsParams p{iterations, playouts, c_explore, (uint32_t)max_tree_nodes, seed, counter * 256u, id_key};
    switch (n) {
#define CASE(K) \
    case K: mcts_n<K>(E, boards, meta, legal, id_base, p, visits, wins2, best, tree_nodes, status); break;
#ifdef MCTS_MAIN  // the sanitizer program's sizes only: one-, two- and four-word nodes, a shorter build
        CASE(4) CASE(6) CASE(8) CASE(10) CASE(16)
#else
        CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#endif
#undef CASE
        default: return -1;
    }
    return 0;
}

extern "C" uint32_t host_mcts_isqrt(uint64_t x) { return mcts_isqrt(x); }

// isqrt of 0, 1, every k*k - 1, k*k, k*k + 1 for k < 65536, and 2^32 - 1 against the definition
// (s*s <= x < (s+1)*(s+1)): the number of arguments that fail
extern "C" int host_mcts_isqrt_sweep(void) {
    int bad = 0;
    auto check = [&](uint64_t x) {
        const uint64_t s = mcts_isqrt(x);
        bad += !(s * s <= x && x < (s + 1) * (s + 1));
    };
    check(0);
    check(1);
    check(0xffffffffull);
    check(0x100000000ull);
    for (uint64_t k = 1; k < 65536; ++k) {
        check(k * k - 1);
        check(k * k);
        check(k * k + 1);
    }
    return bad;
}

#ifdef MCTS_MAIN
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n, E, I, R, C, T, cases = 0, boards_done = 0;
    unsigned long long seed, id_key, id_base, counter;
    while (fscanf(f, "%d %d %d %d %d %d %llu %llu %llu %llu", &n, &E, &I, &R, &C, &T, &seed, &id_key, &id_base,
                  &counter) == 10) {
        if (n < 4 || n > 16 || E < 1) return 2;
        const int W = (n * n + 63) / 64, NN = n * n;
        for (int e = 0; e < E; ++e) {
            int meta, want_status, want_best, want_nodes;
            if (fscanf(f, "%d %d %d %d", &meta, &want_status, &want_best, &want_nodes) != 4) return 2;
            uint64_t b[8] = {0}, lg[4] = {0};
            for (int i = 0; i < 3 * W; ++i) {
                unsigned long long x;
                if (fscanf(f, "%llx", &x) != 1) return 2;
                if (i < 2 * W) b[i] = x;
                else lg[i - 2 * W] = x;
            }
            std::vector<int32_t> want(2 * NN), got(2 * NN, 7);
            for (int a = 0; a < 2 * NN; ++a)
                if (fscanf(f, "%d", &want[a]) != 1) return 2;
            const uint16_t m = (uint16_t)meta;
            int32_t best = 7, nodes = 7;
            uint8_t status = 7;
            if (host_mcts(n, 1, b, &m, lg, (uint32_t)id_base + (uint32_t)e, I, R, C, T, seed, (uint32_t)id_key, counter,
                          got.data(), got.data() + NN, &best, &nodes, &status))
                return 2;
            if (status != want_status || best != want_best || nodes != want_nodes || got != want) {
                fprintf(stderr, "FAILED case %d board %d: status %d best %d tree_nodes %d, expected %d %d %d\n", cases, e,
                        status, best, nodes, want_status, want_best, want_nodes);
                return 1;
            }
            ++boards_done;
        }
        ++cases;
    }
    fclose(f);
    if (!cases) return 2;
    if (host_mcts_isqrt_sweep()) return 1;
    printf("mcts core under ASan and UBSan: %d boards of %d cases clean\n", boards_done, cases);
    return 0;
}
#endif
