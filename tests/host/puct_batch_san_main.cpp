// A stand-alone program for -fsanitize=address,undefined over the batch calls of
// the network-guided search (tests/host/puct_batch_host.cpp, included here: the
// host build of csrc/puct.hpp), for tests/test_puct_batch_sanitizers.py.  It runs
// the searches of a text file whole, E boards at once, in a heap workspace of
// exactly oth_puct_batch_workspace_bytes' size and leaf arrays of exactly E K
// rows, with the tests' hash evaluator (tests/puct_ref.py hash_eval, repeated
// here), then one re-root move, and compares with what tests/puct_batch_ref.py
// recorded.  The file: a header line
//   n E sims C T K launches
// E lines: meta, the black, white and possible_moves words in hex; after every
// launch a line of E K kinds; E lines: status best tree_nodes, N*N visits; then
// the re-root: sim_limit, E lines: action, the handle's meta and 3W words in hex,
// kept, used; and a line of E K kinds.  Test infrastructure only.
#define PUCT_BATCH_MAIN
#include <stdio.h>

#include <vector>

#include "puct_batch_host.cpp"

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

bool read_hex(FILE* f, uint64_t* out, int count) {
    for (int i = 0; i < count; ++i) {
        unsigned long long x;
        if (fscanf(f, "%llx", &x) != 1) return false;
        out[i] = x;
    }
    return true;
}

bool kinds_match(FILE* f, const std::vector<uint8_t>& kind, const char* what, int i) {
    for (size_t r = 0; r < kind.size(); ++r) {
        int want;
        if (fscanf(f, "%d", &want) != 1) return false;
        if (want != kind[r]) {
            fprintf(stderr, "FAILED %s %d row %zu: kind %d, expected %d\n", what, i, r, kind[r], want);
            return false;
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n, E, sims, C, T, K, launches, cases = 0;
    while (fscanf(f, "%d %d %d %d %d %d %d", &n, &E, &sims, &C, &T, &K, &launches) == 7) {
        if (bad(n, E, C, T, K) || sims < 1) return 2;
        const int W = (n * n + 63) / 64, NN = n * n, R = E * K;
        std::vector<uint64_t> boards((size_t)E * 2 * W), legal((size_t)E * W);
        std::vector<uint16_t> meta(E);
        for (int e = 0; e < E; ++e) {
            int m;
            if (fscanf(f, "%d", &m) != 1 || !read_hex(f, &boards[(size_t)e * 2 * W], 2 * W) ||
                !read_hex(f, &legal[(size_t)e * W], W))
                return 2;
            meta[e] = (uint16_t)m;
        }
        // a workspace of exactly the reported size and of garbage, leaf arrays of exactly E K rows
        std::vector<uint64_t> ws(host_puct_batch_ws_words(n, E, T, K), 0xdeadbeefdeadbeefull);
        std::vector<uint8_t> kind(R, 7);
        std::vector<uint64_t> lb((size_t)R * 2 * W, 7), ll((size_t)R * W, 7);
        std::vector<uint16_t> lm(R, 7);
        std::vector<int32_t> priors((size_t)R * NN), values(R);
        if (host_puct_begin_batch(n, E, T, K, boards.data(), meta.data(), legal.data(), ws.data(), kind.data(),
                                  lb.data(), lm.data(), ll.data()))
            return 2;
        for (int i = 0; i < launches; ++i) {
            for (int r = 0; r < R; ++r)
                hash_eval(&lb[(size_t)r * 2 * W], 2 * W, lm[r], NN, &priors[(size_t)r * NN], &values[r]);
            if (host_puct_advance_batch(n, E, T, K, C, ws.data(), priors.data(), values.data(), sims, kind.data(),
                                        lb.data(), lm.data(), ll.data()))
                return 2;
            if (!kinds_match(f, kind, "launch", i)) return 1;
        }
        std::vector<int32_t> visits((size_t)E * NN, 7), best(E, 7), nodes(E, 7);
        std::vector<uint8_t> status(E, 7);
        if (host_puct_batch_result(n, E, T, ws.data(), visits.data(), nullptr, best.data(), nodes.data(), status.data(),
                                   nullptr))
            return 2;
        for (int e = 0; e < E; ++e) {
            int ws_, wb, wn;
            if (fscanf(f, "%d %d %d", &ws_, &wb, &wn) != 3) return 2;
            bool ok = status[e] == ws_ && best[e] == wb && nodes[e] == wn;
            for (int a = 0; a < NN; ++a) {
                int v;
                if (fscanf(f, "%d", &v) != 1) return 2;
                ok = ok && visits[(size_t)e * NN + a] == v;
            }
            if (!ok) {
                fprintf(stderr, "FAILED case %d board %d: status %d best %d tree_nodes %d, expected %d %d %d\n", cases, e,
                        status[e], best[e], nodes[e], ws_, wb, wn);
                return 1;
            }
        }
        // one re-root move
        int lim;
        if (fscanf(f, "%d", &lim) != 1) return 2;
        std::vector<int32_t> actions(E), want_kept(E), want_used(E);
        for (int e = 0; e < E; ++e) {
            int a, m;
            if (fscanf(f, "%d %d", &a, &m) != 2 || !read_hex(f, &boards[(size_t)e * 2 * W], 2 * W) ||
                !read_hex(f, &legal[(size_t)e * W], W) || fscanf(f, "%d %d", &want_kept[e], &want_used[e]) != 2)
                return 2;
            actions[e] = a;
            meta[e] = (uint16_t)m;
        }
        std::vector<uint8_t> kept(E, 7);
        if (host_puct_reroot_batch(n, E, T, K, C, ws.data(), boards.data(), meta.data(), legal.data(), actions.data(),
                                   nullptr, kept.data(), lim, kind.data(), lb.data(), lm.data(), ll.data()))
            return 2;
        if (host_puct_batch_result(n, E, T, ws.data(), visits.data(), nullptr, nullptr, nodes.data(), nullptr, nullptr))
            return 2;
        for (int e = 0; e < E; ++e)
            if (kept[e] != want_kept[e] || nodes[e] != want_used[e]) {
                fprintf(stderr, "FAILED case %d board %d re-root: kept %d used %d, expected %d %d\n", cases, e, kept[e],
                        nodes[e], want_kept[e], want_used[e]);
                return 1;
            }
        if (!kinds_match(f, kind, "re-root", 0)) return 1;
        ++cases;
    }
    fclose(f);
    if (!cases) return 2;
    printf("puct batch calls under ASan and UBSan: %d cases clean\n", cases);
    return 0;
}
