// A stand-alone program for -fsanitize=address,undefined over the play-ntuple core
// (tests/host/play_ntuple_host.cpp, included here: the host build of csrc/play_ntuple.hpp), for
// tests/test_play_ntuple_sanitizers.py.  It runs the cases of a text file on heap buffers of exactly
// the sizes the call is given and compares with what tests/play_ntuple_ref.py recorded.  A case is a
// header line
//   n T value_shift E depth terminal endgame_empties explore max_nodes seed
// then per tuple its length and its squares; the n_weights + 1 weights; and per board the 2W words
// of its boards and the W words of its possible_moves in hex, its meta, its global id, its ply's
// index, and the action, fallback, explored and target expected.
// Test infrastructure only.
#include <stdio.h>

#include <vector>

#define PLAY_NTUPLE_SAN_MAIN 1
#include "play_ntuple_host.cpp"

namespace {

bool read_hex(FILE* f, uint64_t* out, size_t count) {
    for (size_t i = 0; i < count; ++i) {
        unsigned long long x;
        if (fscanf(f, "%llx", &x) != 1) return false;
        out[i] = x;
    }
    return true;
}

template <typename T>
bool same(const std::vector<T>& got, const std::vector<T>& want, const char* what, int c) {
    for (size_t i = 0; i < want.size(); ++i)
        if (got[i] != want[i]) {
            fprintf(stderr, "FAILED case %d: %s[%zu] is %lld, expected %lld\n", c, what, i, (long long)got[i],
                    (long long)want[i]);
            return false;
        }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n, T, shift, E, depth, terminal, endgame, explore, cases = 0;
    unsigned long long max_nodes, seed;
    while (fscanf(f, "%d %d %d %d %d %d %d %d %llu %llu", &n, &T, &shift, &E, &depth, &terminal, &endgame, &explore,
                  &max_nodes, &seed) == 10) {
        if (n < 4 || n > 16 || T < 1 || T > 32 || E < 1) return 2;
        NtupleParams* p = new NtupleParams();  // (on the heap: a read beyond the struct is seen)
        p->tuples = T;
        p->value_shift = shift;
        size_t count = 1;
        for (int t = 0; t < T; ++t) {
            if (fscanf(f, "%d", &p->length[t]) != 1 || p->length[t] < 1 || p->length[t] > 8) return 2;
            for (int i = 0; i < p->length[t]; ++i)
                if (fscanf(f, "%d", &p->squares[t][i]) != 1) return 2;
            count += ntuple_pow3(p->length[t]);
        }
        std::vector<int32_t> w(count);
        for (size_t i = 0; i < count; ++i)
            if (fscanf(f, "%d", &w[i]) != 1) return 2;
        const size_t W = ((size_t)n * n + 63) / 64;
        std::vector<uint64_t> boards((size_t)E * 2 * W), legal((size_t)E * W), g((size_t)E);
        std::vector<uint16_t> meta((size_t)E);
        std::vector<uint32_t> ids((size_t)E);
        std::vector<int32_t> want_a((size_t)E), want_t((size_t)E), act((size_t)E, 7), tgt((size_t)E, 7);
        std::vector<uint8_t> want_f((size_t)E), want_x((size_t)E), fb((size_t)E, 7), ex((size_t)E, 7);
        for (int e = 0; e < E; ++e) {
            int m, wf, wx;
            unsigned long long id, gg;
            if (!read_hex(f, &boards[(size_t)e * 2 * W], 2 * W) || !read_hex(f, &legal[(size_t)e * W], W) ||
                fscanf(f, "%d %llu %llu %d %d %d %d", &m, &id, &gg, &want_a[e], &wf, &wx, &want_t[e]) != 7)
                return 2;
            meta[e] = (uint16_t)m;
            ids[e] = (uint32_t)id;
            g[e] = gg;
            want_f[e] = (uint8_t)wf;
            want_x[e] = (uint8_t)wx;
        }
        if (host_ntuple_move(n, E, boards.data(), meta.data(), legal.data(), p, w.data(), depth, terminal, endgame,
                             explore, max_nodes, seed, ids.data(), g.data(), act.data(), fb.data(), ex.data(),
                             tgt.data()))
            return 2;
        const bool ok = same(act, want_a, "actions", cases) && same(fb, want_f, "fallbacks", cases) &&
                        same(ex, want_x, "explored", cases) && same(tgt, want_t, "targets", cases);
        delete p;
        if (!ok) return 1;
        ++cases;
    }
    fclose(f);
    if (!cases) return 2;
    printf("play-ntuple core under ASan and UBSan: %d cases clean\n", cases);
    return 0;
}
