// Host build of the self-play calls of the network-guided search (csrc/puct.hpp:
// puct_pick_board and puct_reroot_board, the text the device kernels run,
// compiled with g++) for tests/test_puct_play_host.py: as a shared library with C
// linkage that has oth_puct_pick and oth_puct_reroot on a host workspace (begin,
// advance and result come from tests/host/puct_host.cpp: the workspace is the
// same), and, with -DPUCT_PLAY_MAIN, as a stand-alone program for
// -fsanitize=address,undefined that plays the games of a text file board by
// board with the tests' hash evaluator and compares every output with what
// tests/puct_play_ref.py recorded.  The file: a header line
//   n E S M C T seed id_key
// then for every board a line
//   e sample meta, the black, white and possible_moves words in hex
// and M lines, one a move:
//   counter want_pick want_best want_nodes, N*N visits, action, the handle's meta
//   and its 3W words in hex after the step, has_priors and then N*N root priors,
//   want_kept want_used want_kind want_leaf_meta (after the re-root).
// Test infrastructure only.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../gymothelloenv_amd/csrc/puct.hpp"

using namespace oth;

namespace {

template <int N>
void pick_n(uint32_t E, uint32_t T, uint64_t* wsp, const uint8_t* sample, uint64_t seed, uint32_t id_key,
            uint32_t id_base, uint64_t counter, int32_t* actions) {
    const PuctWs<N> ws{wsp, E, T};
    if (*ws.tag() != puct_tag(N, E, T)) return;
    for (uint32_t e = 0; e < E; ++e)
        actions[e] = puct_pick_board<N>(ws, e, sample && sample[e], seed, id_key + id_base + e, counter);
}

template <int N>
void reroot_n(uint32_t E, uint32_t T, int C, uint64_t* wsp, const uint64_t* boards, const uint16_t* meta,
              const uint64_t* legal, const int32_t* actions, const int32_t* root_priors, uint8_t* kept,
              const PuctLeaves& out) {
    constexpr int W = Geo<N>::W;
    const PuctWs<N> ws{wsp, E, T};
    if (*ws.tag() != puct_tag(N, E, T)) return;
    for (uint32_t e = 0; e < E; ++e)
        puct_reroot_board<N>(ws, e, C, boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W,
                             legal + (size_t)e * W, meta[e], actions[e],
                             root_priors ? root_priors + (size_t)e * N * N : nullptr, kept ? kept + e : nullptr, out);
}

bool bad(int n, int E, int C, int T) {
    return n < 4 || n > 16 || E < 1 || C < 0 || C > PUCT_MAX_C || T < n * n || T > PUCT_MAX_TREE_NODES;
}

}  // namespace

#ifdef PUCT_PLAY_MAIN  // the sanitizer program's sizes only: one- and two-word nodes, a shorter build
#define SIZES(X) X(4) X(8) X(10)
#else
#define SIZES(X) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
#endif

extern "C" int host_puct_pick(int n, int E, int T, uint64_t* ws, const uint8_t* sample, uint64_t seed, uint32_t id_key,
                              uint32_t id_base, uint64_t counter, int32_t* actions) {
    if (bad(n, E, 0, T) || !actions) return -1;
    switch (n) {
#define CASE(K) \
    case K: pick_n<K>((uint32_t)E, (uint32_t)T, ws, sample, seed, id_key, id_base, counter, actions); break;
        SIZES(CASE)
#undef CASE
        default: return -1;
    }
    return 0;
}

extern "C" int host_puct_reroot(int n, int E, int T, int C, uint64_t* ws, const uint64_t* boards, const uint16_t* meta,
                                const uint64_t* legal, const int32_t* actions, const int32_t* root_priors,
                                uint8_t* kept, uint8_t* kind, uint64_t* lboards, uint16_t* lmeta, uint64_t* llegal) {
    if (bad(n, E, C, T) || !actions) return -1;
    const PuctLeaves out{kind, lboards, lmeta, llegal};
    switch (n) {
#define CASE(K) \
    case K: reroot_n<K>((uint32_t)E, (uint32_t)T, C, ws, boards, meta, legal, actions, root_priors, kept, out); break;
        SIZES(CASE)
#undef CASE
        default: return -1;
    }
    return 0;
}

#ifdef PUCT_PLAY_MAIN
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

template <int N>
int begin_one(uint32_t T, const uint64_t* b, uint16_t meta, const uint64_t* lg, uint64_t* wsp, const PuctLeaves& out) {
    constexpr int W = Geo<N>::W;
    const PuctWs<N> ws{wsp, 1u, T};
    *ws.tag() = puct_tag(N, 1u, T);
    puct_begin_board<N>(ws, 0u, b, b + W, lg, meta, out);
    return 0;
}
template <int N>
int advance_one(uint32_t T, int C, uint64_t* wsp, const int32_t* priors, int32_t value, const PuctLeaves& out) {
    puct_advance_board<N>(PuctWs<N>{wsp, 1u, T}, 0u, C, priors, value, true, out);
    return 0;
}
template <int N>
int result_one(uint32_t T, uint64_t* wsp, int32_t* visits, int32_t* best, int32_t* nodes) {
    puct_result_board<N>(PuctWs<N>{wsp, 1u, T}, 0u, visits, nullptr, best, nodes, nullptr);
    return 0;
}

#define DISPATCH(n, CALL)            \
    switch (n) {                     \
        case 4: CALL(4); break;      \
        case 8: CALL(8); break;      \
        case 10: CALL(10); break;    \
        default: return 2;           \
    }

bool read_hex(FILE* f, uint64_t* out, int count) {
    for (int i = 0; i < count; ++i) {
        unsigned long long x;
        if (fscanf(f, "%llx", &x) != 1) return false;
        out[i] = x;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n, E, S, M, C, T, cases = 0, boards_done = 0;
    unsigned long long seed, id_key;
    while (fscanf(f, "%d %d %d %d %d %d %llu %llu", &n, &E, &S, &M, &C, &T, &seed, &id_key) == 8) {
        if (bad(n, E, C, T) || S < 1 || M < 1) return 2;
        const int W = (n * n + 63) / 64, NN = n * n;
        for (int b = 0; b < E; ++b) {
            int e, sample, meta;
            if (fscanf(f, "%d %d %d", &e, &sample, &meta) != 3) return 2;
            uint64_t pos[12];
            if (!read_hex(f, pos, 3 * W)) return 2;
            // one board a search, in a workspace of exactly the reported size and of garbage
            std::vector<uint64_t> ws(puct_ws_words(n, 1, (uint64_t)T), 0xdeadbeefdeadbeefull);
            uint8_t kind = 7;
            uint64_t lb[8], ll[4];
            uint16_t lm = 7;
            const PuctLeaves out{&kind, lb, &lm, ll};
            std::vector<int32_t> priors(NN), visits(NN), want_v(NN), rp(NN);
            int32_t value;
#define BEGIN(K) begin_one<K>((uint32_t)T, pos, (uint16_t)meta, pos + 2 * W, ws.data(), out)
            DISPATCH(n, BEGIN)
            for (int m = 0; m < M; ++m) {
                unsigned long long counter;
                int want_pick, want_best, want_nodes, action, hmeta, has_priors, want_kept, want_used, want_kind, want_lm;
                if (fscanf(f, "%llu %d %d %d", &counter, &want_pick, &want_best, &want_nodes) != 4) return 2;
                for (int a = 0; a < NN; ++a)
                    if (fscanf(f, "%d", &want_v[a]) != 1) return 2;
                uint64_t hpos[12];
                if (fscanf(f, "%d %d", &action, &hmeta) != 2 || !read_hex(f, hpos, 3 * W)) return 2;
                if (fscanf(f, "%d", &has_priors) != 1) return 2;
                if (has_priors)
                    for (int a = 0; a < NN; ++a)
                        if (fscanf(f, "%d", &rp[a]) != 1) return 2;
                if (fscanf(f, "%d %d %d %d", &want_kept, &want_used, &want_kind, &want_lm) != 4) return 2;
                for (int i = 0; i < S; ++i) {
                    hash_eval(lb, 2 * W, lm, NN, priors.data(), &value);
#define ADVANCE(K) advance_one<K>((uint32_t)T, C, ws.data(), priors.data(), value, out)
                    DISPATCH(n, ADVANCE)
                }
                int32_t best = 7, nodes = 7, got_pick = 7;
#define RESULT(K) result_one<K>((uint32_t)T, ws.data(), visits.data(), &best, &nodes)
                DISPATCH(n, RESULT)
                const uint8_t smp = (uint8_t)sample;
                if (host_puct_pick(n, 1, T, ws.data(), &smp, seed, (uint32_t)id_key, (uint32_t)e, counter, &got_pick))
                    return 2;
                if (got_pick != want_pick || best != want_best || nodes != want_nodes || visits != want_v) {
                    fprintf(stderr, "FAILED case %d board %d move %d: pick %d best %d tree_nodes %d, expected %d %d %d\n",
                            cases, e, m, got_pick, best, nodes, want_pick, want_best, want_nodes);
                    return 1;
                }
                const uint16_t hm = (uint16_t)hmeta;
                const int32_t act = action;
                uint8_t kept = 7;
                if (host_puct_reroot(n, 1, T, C, ws.data(), hpos, &hm, hpos + 2 * W, &act,
                                     has_priors ? rp.data() : nullptr, &kept, &kind, lb, &lm, ll))
                    return 2;
                DISPATCH(n, RESULT)
                if (kept != want_kept || nodes != want_used || kind != want_kind || lm != want_lm) {
                    fprintf(stderr, "FAILED case %d board %d move %d: kept %d used %d kind %d meta %d, expected %d %d %d %d\n",
                            cases, e, m, kept, nodes, kind, lm, want_kept, want_used, want_kind, want_lm);
                    return 1;
                }
            }
            ++boards_done;
        }
        ++cases;
    }
    fclose(f);
    if (!cases) return 2;
    printf("puct pick and reroot under ASan and UBSan: %d boards of %d cases clean\n", boards_done, cases);
    return 0;
}
#endif
