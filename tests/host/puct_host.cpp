// Host build of the network-guided search's core (csrc/puct.hpp: the layout, the
// key, begin / apply / select / leaf / outputs that the device kernels run,
// compiled with g++) for tests/test_puct_host.py: as a shared library with C
// linkage that has the library's three calls on a host workspace, and, with
// -DPUCT_MAIN, as a stand-alone program for -fsanitize=address,undefined that
// searches the boards of a text file with the tests' hash evaluator
// (tests/puct_ref.py hash_eval, repeated here) and compares every output (a
// header line: n E sims C T; then one board a line: meta status best
// tree_nodes, the black, white and possible_moves words in hex, then N*N visits
// and N*N value sums).  Test infrastructure only.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../gymothelloenv_amd/csrc/puct.hpp"

using namespace oth;

namespace {

template <int N>
void begin_n(uint32_t E, uint32_t T, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal, uint64_t* wsp,
             const PuctLeaves& out) {
    constexpr int W = Geo<N>::W;
    const PuctWs<N> ws{wsp, E, T};
    *ws.tag() = puct_tag(N, E, T);
    for (uint32_t e = 0; e < E; ++e)
        puct_begin_board<N>(ws, e, boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W, legal + (size_t)e * W,
                            meta[e], out);
}

template <int N>
void advance_n(uint32_t E, uint32_t T, int C, uint64_t* wsp, const int32_t* priors, const int32_t* values, int more,
               const PuctLeaves& out) {
    const PuctWs<N> ws{wsp, E, T};
    if (*ws.tag() != puct_tag(N, E, T)) return;
    for (uint32_t e = 0; e < E; ++e)
        puct_advance_board<N>(ws, e, C, priors + (size_t)e * N * N, values[e], more != 0, out);
}

template <int N>
void result_n(uint32_t E, uint32_t T, uint64_t* wsp, int32_t* visits, int64_t* sums, int32_t* best, int32_t* nodes,
              uint8_t* status) {
    const PuctWs<N> ws{wsp, E, T};
    if (*ws.tag() != puct_tag(N, E, T)) return;
    for (uint32_t e = 0; e < E; ++e)
        puct_result_board<N>(ws, e, visits + (size_t)e * N * N, sums ? sums + (size_t)e * N * N : nullptr,
                             best ? best + e : nullptr, nodes ? nodes + e : nullptr, status ? status + e : nullptr);
}

bool bad(int n, int E, int C, int T) {
    return n < 4 || n > 16 || E < 1 || C < 0 || C > PUCT_MAX_C || T < n * n || T > PUCT_MAX_TREE_NODES;
}

}  // namespace

#ifdef PUCT_MAIN  // the sanitizer program's sizes only: one-, two- and four-word nodes, a shorter build
#define SIZES(X) X(4) X(6) X(8) X(10) X(16)
#else
#define SIZES(X) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
#endif

extern "C" uint64_t host_puct_ws_words(int n, int E, int T) { return puct_ws_words(n, (uint64_t)E, (uint64_t)T); }

extern "C" int host_puct_begin(int n, int E, int T, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal,
                               uint64_t* ws, uint8_t* kind, uint64_t* lboards, uint16_t* lmeta, uint64_t* llegal) {
    if (bad(n, E, 0, T)) return -1;
    const PuctLeaves out{kind, lboards, lmeta, llegal};
    switch (n) {
#define CASE(K) \
    case K: begin_n<K>((uint32_t)E, (uint32_t)T, boards, meta, legal, ws, out); break;
        SIZES(CASE)
#undef CASE
        default: return -1;
    }
    return 0;
}

extern "C" int host_puct_advance(int n, int E, int T, int C, uint64_t* ws, const int32_t* priors,
                                 const int32_t* values, int more, uint8_t* kind, uint64_t* lboards, uint16_t* lmeta,
                                 uint64_t* llegal) {
    if (bad(n, E, C, T)) return -1;
    const PuctLeaves out{kind, lboards, lmeta, llegal};
    switch (n) {
#define CASE(K) \
    case K: advance_n<K>((uint32_t)E, (uint32_t)T, C, ws, priors, values, more, out); break;
        SIZES(CASE)
#undef CASE
        default: return -1;
    }
    return 0;
}

extern "C" int host_puct_result(int n, int E, int T, uint64_t* ws, int32_t* visits, int64_t* sums, int32_t* best,
                                int32_t* nodes, uint8_t* status) {
    if (bad(n, E, 0, T)) return -1;
    switch (n) {
#define CASE(K) \
    case K: result_n<K>((uint32_t)E, (uint32_t)T, ws, visits, sums, best, nodes, status); break;
        SIZES(CASE)
#undef CASE
        default: return -1;
    }
    return 0;
}

extern "C" int64_t host_puct_key(int64_t w_c, uint32_t v_c, uint32_t P_c, uint32_t v_p, int C) {
    return puct_key(w_c, v_c, P_c, (uint64_t)(uint32_t)C * mcts_isqrt((uint64_t)v_p << 16));
}

#ifdef PUCT_MAIN
namespace {

uint64_t mix(uint64_t h) {
    h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
    h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
    return h ^ (h >> 31);
}

// puct_ref.hash_eval of one leaf
void hash_eval(const uint64_t* boards, int words, uint16_t meta, int NN, int32_t* priors, int32_t* value) {
    uint64_t h = mix((uint64_t)meta + 0x9E3779B97F4A7C15ull);
    for (int j = 0; j < words; ++j) h = mix(h ^ boards[j] ^ (uint64_t)(j + 1));
    for (int a = 0; a < NN; ++a)
        priors[a] = (int32_t)(mix(h + ((uint64_t)a + 1u) * 0xD1342543DE82EF95ull) % 70000u) - 2000;
    *value = (int32_t)(mix(h ^ 0xA0761D6478BD642Full) % 70001u) - 35000;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n, E, sims, C, T, cases = 0, boards_done = 0;
    while (fscanf(f, "%d %d %d %d %d", &n, &E, &sims, &C, &T) == 5) {
        if (bad(n, E, C, T) || sims < 1) return 2;
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
            std::vector<int32_t> want_v(NN), got_v(NN, 7);
            std::vector<int64_t> want_w(NN), got_w(NN, 7);
            for (int a = 0; a < NN; ++a)
                if (fscanf(f, "%d", &want_v[a]) != 1) return 2;
            for (int a = 0; a < NN; ++a) {
                long long x;
                if (fscanf(f, "%lld", &x) != 1) return 2;
                want_w[a] = x;
            }
            // one board a search, in a workspace of exactly the reported size and of garbage
            std::vector<uint64_t> ws(host_puct_ws_words(n, 1, T), 0xdeadbeefdeadbeefull);
            const uint16_t m = (uint16_t)meta;
            uint8_t kind = 7;
            uint64_t lb[8], ll[4];
            uint16_t lm = 7;
            std::vector<int32_t> priors(NN);
            int32_t value;
            if (host_puct_begin(n, 1, T, b, &m, lg, ws.data(), &kind, lb, &lm, ll)) return 2;
            for (int i = 0; i < sims; ++i) {
                hash_eval(lb, 2 * W, lm, NN, priors.data(), &value);
                if (host_puct_advance(n, 1, T, C, ws.data(), priors.data(), &value, i < sims - 1, &kind, lb, &lm, ll))
                    return 2;
            }
            int32_t best = 7, nodes = 7;
            uint8_t status = 7;
            if (host_puct_result(n, 1, T, ws.data(), got_v.data(), got_w.data(), &best, &nodes, &status)) return 2;
            if (status != want_status || best != want_best || nodes != want_nodes || got_v != want_v ||
                got_w != want_w || kind != PUCT_LEAF_NONE) {
                fprintf(stderr, "FAILED case %d board %d: status %d best %d tree_nodes %d, expected %d %d %d\n", cases,
                        e, status, best, nodes, want_status, want_best, want_nodes);
                return 1;
            }
            ++boards_done;
        }
        ++cases;
    }
    fclose(f);
    if (!cases) return 2;
    printf("puct core under ASan and UBSan: %d boards of %d cases clean\n", boards_done, cases);
    return 0;
}
#endif
