// A stand-alone program for -fsanitize=address,undefined over the root noise
// (tests/host/noise_host.cpp, included here: the host build of csrc/noise.hpp), for
// tests/test_noise_sanitizers.py.  It runs the cases of a text file on heap buffers of
// exactly the sizes the call is given and compares with what tests/noise_ref.py
// recorded.  A case: a header line
//   n E K leaf inplace epsilon seed id0 counter
// the 4,096 table entries in hex; per board the 2W words of the handle's board and the W
// words of its possible_moves in hex; in leaf mode per row its kind and the 2W words of
// its leaf board; the E K N*N priors; the E K N*N expected outputs.  Test infrastructure
// only.
#include <stdio.h>

#include <vector>

#include "noise_host.cpp"

namespace {

bool read_hex(FILE* f, uint64_t* out, size_t count) {
    for (size_t i = 0; i < count; ++i) {
        unsigned long long x;
        if (fscanf(f, "%llx", &x) != 1) return false;
        out[i] = x;
    }
    return true;
}

bool read_ints(FILE* f, int32_t* out, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (fscanf(f, "%d", &out[i]) != 1) return false;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n, E, K, leaf, inplace, epsilon, cases = 0;
    unsigned long long seed, id0, counter;
    while (fscanf(f, "%d %d %d %d %d %d %llu %llu %llu", &n, &E, &K, &leaf, &inplace, &epsilon, &seed, &id0, &counter) == 9) {
        if (n < 4 || n > 16 || E < 1 || K < 1 || K > 64) return 2;
        const size_t nn = (size_t)n * n, W = (nn + 63) / 64, R = (size_t)E * K;
        std::vector<uint64_t> t64(NOISE_TABLE);
        if (!read_hex(f, t64.data(), t64.size())) return 2;
        std::vector<uint32_t> table(t64.begin(), t64.end());
        std::vector<uint64_t> hb((size_t)E * 2 * W), hl((size_t)E * W);
        for (int e = 0; e < E; ++e)
            if (!read_hex(f, &hb[(size_t)e * 2 * W], 2 * W) || !read_hex(f, &hl[(size_t)e * W], W)) return 2;
        std::vector<uint8_t> kind(leaf ? R : 0);
        std::vector<uint64_t> boards(leaf ? R * 2 * W : 0);
        for (size_t r = 0; leaf && r < R; ++r) {
            int k;
            if (fscanf(f, "%d", &k) != 1 || !read_hex(f, &boards[r * 2 * W], 2 * W)) return 2;
            kind[r] = (uint8_t)k;
        }
        std::vector<int32_t> in(R * nn), want(R * nn);
        if (!read_ints(f, in.data(), in.size()) || !read_ints(f, want.data(), want.size())) return 2;
        std::vector<int32_t> out = inplace ? in : std::vector<int32_t>(R * nn, 7);
        if (host_puct_noise(n, E, K, hb.data(), hl.data(), leaf ? kind.data() : nullptr, leaf ? boards.data() : nullptr,
                            inplace ? out.data() : in.data(), out.data(), epsilon, table.data(), seed, (uint32_t)id0,
                            counter))
            return 2;
        for (size_t i = 0; i < out.size(); ++i)
            if (out[i] != want[i]) {
                fprintf(stderr, "FAILED case %d row %zu square %zu: %d, expected %d\n", cases, i / nn, i % nn, out[i],
                        want[i]);
                return 1;
            }
        ++cases;
    }
    fclose(f);
    if (!cases) return 2;
    printf("root noise under ASan and UBSan: %d cases clean\n", cases);
    return 0;
}
