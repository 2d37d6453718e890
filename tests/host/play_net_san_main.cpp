// A stand-alone program for -fsanitize=address,undefined over the network's move
// (tests/host/play_net_host.cpp, included here: the host build of csrc/play_net.hpp over
// csrc/net.hpp), for tests/test_play_net_sanitizers.py.  It packs the weights of a text
// file into a heap blob of exactly oth_net_blob_bytes' size, computes the moves of the
// rows into an array of exactly R elements and compares with what tests/play_net_ref.py
// recorded.  The file: a line
//   n L H shift0 shift1 shift2 shift3 policy_shift value_shift R seed id_base g0 K
// then the weights, the biases, per row a line (meta, the 3W words in hex), and K lines
// (sample_discs, R moves); row r draws with id id_base + r and ply index g0 + r.
// Test infrastructure only.
#include <stdio.h>

#include <vector>

#include "play_net_host.cpp"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int n, R, K, cases = 0;
    unsigned long long seed, g0;
    unsigned id_base;
    NetParams p;
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %llu %u %llu %d", &n, &p.layers, &p.width, &p.shift[0], &p.shift[1],
                  &p.shift[2], &p.shift[3], &p.policy_shift, &p.value_shift, &R, &seed, &id_base, &g0, &K) == 14) {
        if (net_check(n, &p) || R < 1 || K < 1) return 2;
        const uint64_t bytes = net_geo(n, p).bytes();
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
        if (net_pack(n, p, w.data(), b.data(), blob.data())) return 2;
        std::vector<uint64_t> boards((size_t)R * 2 * W), legal((size_t)R * W), g(R);
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
            g[r] = g0 + (uint64_t)r;
        }
        for (int k = 0; k < K; ++k) {
            int sample_discs;
            if (fscanf(f, "%d", &sample_discs) != 1) return 2;
            std::vector<int32_t> moves(R, 7);
            if (host_net_moves(n, &p, R, blob.data(), boards.data(), meta.data(), legal.data(), sample_discs, seed,
                               id_base, g.data(), moves.data()))
                return 2;
            for (int r = 0; r < R; ++r) {
                int x;
                if (fscanf(f, "%d", &x) != 1 || x != moves[r]) {
                    fprintf(stderr, "FAILED case %d sample_discs %d row %d\n", cases, sample_discs, r);
                    return 1;
                }
            }
        }
        ++cases;
    }
    fclose(f);
    if (!cases) return 2;
    printf("network moves under ASan and UBSan: %d cases clean\n", cases);
    return 0;
}
