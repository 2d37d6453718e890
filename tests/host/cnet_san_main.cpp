// A stand-alone program for -fsanitize=address,undefined over the convolutional network
// (tests/host/cnet_host.cpp, included here: the host build of csrc/cnet.hpp), for
// tests/test_cnet_sanitizers.py.  It packs the weights of a text file into a heap blob of
// exactly oth_cnet_blob_bytes' size, evaluates the rows into arrays of exactly R rows and
// compares with what tests/cnet_ref.py recorded.  The file: a line
//   n C B shift_stem shift[0 .. 15] shift_head policy_shift value_shift R
// then the weights, the biases, per row a line (meta, the 3W words in hex), and per row a
// line (value, nn priors, nn + 1 logits).  Test infrastructure only.
#include <stdio.h>

#include <vector>

#include "cnet_host.cpp"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n, R, cases = 0;
    CnetParams p;
    while (fscanf(f, "%d %d %d %d", &n, &p.channels, &p.blocks, &p.shift_stem) == 4) {
        for (int l = 0; l < 16; ++l)
            if (fscanf(f, "%d", &p.shift[l]) != 1) return 2;
        if (fscanf(f, "%d %d %d %d", &p.shift_head, &p.policy_shift, &p.value_shift, &R) != 4) return 2;
        const uint64_t bytes = host_cnet_blob_bytes(n, &p);
        if (!bytes || R < 1) return 2;
        const int nn = n * n, W = (nn + 63) / 64;
        std::vector<int8_t> w((size_t)host_cnet_weights(n, &p));
        std::vector<int32_t> b((size_t)host_cnet_biases(n, &p));
        for (size_t i = 0; i < w.size(); ++i) {
            int x;
            if (fscanf(f, "%d", &x) != 1) return 2;
            w[i] = (int8_t)x;
        }
        for (size_t i = 0; i < b.size(); ++i)
            if (fscanf(f, "%d", &b[i]) != 1) return 2;
        std::vector<uint8_t> blob(bytes, 0xa5);
        if (host_cnet_pack(n, &p, w.data(), b.data(), blob.data())) return 2;
        std::vector<uint64_t> boards((size_t)R * 2 * W), legal((size_t)R * W);
        std::vector<uint16_t> meta(R);
        for (int r = 0; r < R; ++r) {
            int mt;
            unsigned long long x;
            if (fscanf(f, "%d", &mt) != 1) return 2;
            meta[r] = (uint16_t)mt;
            for (int j = 0; j < 3 * W; ++j) {
                if (fscanf(f, "%llx", &x) != 1) return 2;
                (j < 2 * W ? boards[(size_t)r * 2 * W + j] : legal[(size_t)r * W + j - 2 * W]) = x;
            }
        }
        std::vector<int32_t> priors((size_t)R * nn, 7), values(R, 7), logits((size_t)R * (nn + 1), 7);
        if (host_cnet_eval(n, &p, R, blob.data(), boards.data(), meta.data(), legal.data(), priors.data(), values.data(),
                           logits.data()))
            return 2;
        std::vector<int32_t> again((size_t)R * nn, 7);  // without the logits
        if (host_cnet_eval(n, &p, R, blob.data(), boards.data(), meta.data(), legal.data(), again.data(), values.data(),
                           nullptr))
            return 2;
        if (again != priors) return 1;
        // a blob of other shifts writes nothing
        CnetParams other = p;
        other.shift_head = p.shift_head ? p.shift_head - 1 : 1;
        std::vector<int32_t> none((size_t)R * nn, 7), nov(R, 7);
        if (host_cnet_eval(n, &other, R, blob.data(), boards.data(), meta.data(), legal.data(), none.data(), nov.data(),
                           nullptr) != 2)
            return 1;
        for (int32_t x : none)
            if (x != 7) return 1;
        for (int r = 0; r < R; ++r) {
            int x;
            bool ok = fscanf(f, "%d", &x) == 1 && x == values[r];
            for (int a = 0; a < nn && ok; ++a) ok = fscanf(f, "%d", &x) == 1 && x == priors[(size_t)r * nn + a];
            for (int o = 0; o <= nn && ok; ++o) ok = fscanf(f, "%d", &x) == 1 && x == logits[(size_t)r * (nn + 1) + o];
            if (!ok) {
                fprintf(stderr, "FAILED case %d row %d\n", cases, r);
                return 1;
            }
        }
        ++cases;
    }
    fclose(f);
    if (!cases) return 2;
    printf("convolutional network under ASan and UBSan: %d cases clean\n", cases);
    return 0;
}
