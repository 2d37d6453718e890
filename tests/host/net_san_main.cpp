// A stand-alone program for -fsanitize=address,undefined over the network
// (tests/host/net_host.cpp, included here: the host build of csrc/net.hpp), for
// tests/test_net_sanitizers.py.  It packs the weights of a text file into a heap
// blob of exactly oth_net_blob_bytes' size, evaluates the rows into arrays of
// exactly R rows and compares with what tests/net_ref.py recorded.  The file: a line
//   n L H shift0 shift1 shift2 shift3 policy_shift value_shift R
// then the weights, the biases, per row a line (meta, the 3W words in hex), and per
// row a line (value, nn priors, nn + 1 logits).  Test infrastructure only.
#include <stdio.h>

#include <vector>

#include "net_host.cpp"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n, R, cases = 0;
    NetParams p;
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d", &n, &p.layers, &p.width, &p.shift[0], &p.shift[1], &p.shift[2],
                  &p.shift[3], &p.policy_shift, &p.value_shift, &R) == 10) {
        const uint64_t bytes = host_net_blob_bytes(n, &p);
        if (!bytes || R < 1) return 2;
        const int nn = n * n, W = (nn + 63) / 64, L = p.layers, H = p.width;
        std::vector<int8_t> w((size_t)H * 3 * nn + (size_t)(L - 1) * H * H + (size_t)(nn + 1) * H);
        std::vector<int32_t> b((size_t)L * H + nn + 1);
        for (size_t i = 0; i < w.size(); ++i) {
            int x;
            if (fscanf(f, "%d", &x) != 1) return 2;
            w[i] = (int8_t)x;
        }
        for (size_t i = 0; i < b.size(); ++i)
            if (fscanf(f, "%d", &b[i]) != 1) return 2;
        std::vector<uint8_t> blob(bytes, 0xa5);
        if (host_net_pack(n, &p, w.data(), b.data(), blob.data())) return 2;
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
        if (host_net_eval(n, &p, R, blob.data(), boards.data(), meta.data(), legal.data(), priors.data(), values.data(),
                          logits.data()))
            return 2;
        std::vector<int32_t> again((size_t)R * nn, 7);  // without the logits
        if (host_net_eval(n, &p, R, blob.data(), boards.data(), meta.data(), legal.data(), again.data(), values.data(),
                          nullptr))
            return 2;
        if (again != priors) return 1;
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
    printf("network under ASan and UBSan: %d cases clean\n", cases);
    return 0;
}
