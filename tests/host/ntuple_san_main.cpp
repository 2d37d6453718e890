// A stand-alone program for -fsanitize=address,undefined over the n-tuple network
// (tests/host/ntuple_host.cpp, included here: the host build of csrc/ntuple.hpp), for
// tests/test_ntuple_sanitizers.py.  It runs the cases of a text file on heap buffers of exactly
// the sizes the calls are given and compares with what tests/ntuple_ref.py recorded.  A case is
// a header line
//   kind n T value_shift R
// then per tuple its length and its squares; the n_weights + 1 weights; per row the 2W words of
// its boards in hex and its meta; and for
//   kind 0 (eval)    the R values and the R sums expected;
//   kind 1 (update)  a line `rate rate_shift`, the R targets, the R deltas and the n_weights + 1
//                    weights expected;
//   kind 2 (search)  a line `depth terminal max_nodes`, per row the W words of its
//                    possible_moves in hex, then per row value, best, status, nodes and the N*N
//                    move_values expected.
// Test infrastructure only.
#include <stdio.h>

#include <vector>

#define NTUPLE_SAN_MAIN 1
#include "ntuple_host.cpp"

namespace {

bool read_hex(FILE* f, uint64_t* out, size_t count) {
    for (size_t i = 0; i < count; ++i) {
        unsigned long long x;
        if (fscanf(f, "%llx", &x) != 1) return false;
        out[i] = x;
    }
    return true;
}

bool read_i32(FILE* f, int32_t* out, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (fscanf(f, "%d", &out[i]) != 1) return false;
    return true;
}

bool read_i64(FILE* f, int64_t* out, size_t count) {
    for (size_t i = 0; i < count; ++i) {
        long long x;
        if (fscanf(f, "%lld", &x) != 1) return false;
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
    int kind, n, T, shift, R, cases = 0;
    while (fscanf(f, "%d %d %d %d %d", &kind, &n, &T, &shift, &R) == 5) {
        if (n < 4 || n > 16 || T < 1 || T > 32 || R < 0) return 2;
        NtupleParams* p = new NtupleParams();  // (on the heap: a read beyond the struct is seen)
        p->tuples = T;
        p->value_shift = shift;
        for (int t = 0; t < T; ++t) {
            if (fscanf(f, "%d", &p->length[t]) != 1 || p->length[t] < 1 || p->length[t] > 8) return 2;
            if (!read_i32(f, p->squares[t], (size_t)p->length[t])) return 2;
        }
        const size_t nn = (size_t)n * n, W = (nn + 63) / 64, count = (size_t)host_ntuple_weight_count(n, p);
        if (!count) return 2;
        std::vector<int32_t> w(count);
        if (!read_i32(f, w.data(), count)) return 2;
        std::vector<uint64_t> boards((size_t)R * 2 * W);
        std::vector<uint16_t> meta((size_t)R);
        for (int r = 0; r < R; ++r) {
            int m;
            if (!read_hex(f, &boards[(size_t)r * 2 * W], 2 * W) || fscanf(f, "%d", &m) != 1) return 2;
            meta[r] = (uint16_t)m;
        }
        bool ok = true;
        if (kind == 0) {
            std::vector<int32_t> want_v((size_t)R), values((size_t)R, 7);
            std::vector<int64_t> want_s((size_t)R), sums((size_t)R, 7);
            if (!read_i32(f, want_v.data(), want_v.size()) || !read_i64(f, want_s.data(), want_s.size())) return 2;
            if (host_ntuple_eval(n, R, p, w.data(), boards.data(), meta.data(), values.data(), sums.data())) return 2;
            ok = same(values, want_v, "values", cases) && same(sums, want_s, "sums", cases);
        } else if (kind == 1) {
            int rate, rate_shift;
            if (fscanf(f, "%d %d", &rate, &rate_shift) != 2) return 2;
            std::vector<int32_t> targets((size_t)R), want_d((size_t)R), deltas((size_t)R, 7), want_w(count);
            if (!read_i32(f, targets.data(), targets.size()) || !read_i32(f, want_d.data(), want_d.size()) ||
                !read_i32(f, want_w.data(), count))
                return 2;
            if (host_ntuple_update(n, R, p, w.data(), boards.data(), meta.data(), targets.data(), rate, rate_shift,
                                   deltas.data()))
                return 2;
            ok = same(deltas, want_d, "deltas", cases) && same(w, want_w, "weights", cases);
        } else if (kind == 2) {
            int depth, terminal;
            unsigned long long max_nodes;
            if (fscanf(f, "%d %d %llu", &depth, &terminal, &max_nodes) != 3) return 2;
            std::vector<uint64_t> legal((size_t)R * W);
            if (!read_hex(f, legal.data(), legal.size())) return 2;
            std::vector<int32_t> want_v((size_t)R), want_b((size_t)R), want_mv((size_t)R * nn);
            std::vector<uint8_t> want_st((size_t)R);
            std::vector<uint64_t> want_nd((size_t)R);
            for (int r = 0; r < R; ++r) {
                int st;
                unsigned long long nd;
                if (fscanf(f, "%d %d %d %llu", &want_v[r], &want_b[r], &st, &nd) != 4) return 2;
                want_st[r] = (uint8_t)st;
                want_nd[r] = nd;
                if (!read_i32(f, &want_mv[(size_t)r * nn], nn)) return 2;
            }
            std::vector<int32_t> value((size_t)R, 7), best((size_t)R, 7), mv((size_t)R * nn, 7);
            std::vector<uint8_t> status((size_t)R, 7);
            std::vector<uint64_t> nodes((size_t)R, 7);
            if (host_search_ntuple(n, R, boards.data(), meta.data(), legal.data(), depth, p, w.data(), terminal, max_nodes,
                                   value.data(), best.data(), mv.data(), status.data(), nodes.data()))
                return 2;
            ok = same(value, want_v, "value", cases) && same(best, want_b, "best", cases) &&
                 same(mv, want_mv, "move_values", cases) && same(status, want_st, "status", cases) &&
                 same(nodes, want_nd, "nodes", cases);
        } else {
            return 2;
        }
        delete p;
        if (!ok) return 1;
        ++cases;
    }
    fclose(f);
    if (!cases) return 2;
    printf("n-tuple network under ASan and UBSan: %d cases clean\n", cases);
    return 0;
}
