// A stand-alone program for -fsanitize=address,undefined over the replay store
// (tests/host/replay_host.cpp, included here: the host build of csrc/replay.hpp),
// for tests/test_replay_sanitizers.py.  It replays the moves of a text file into a
// heap workspace of exactly oth_replay_workspace_bytes' size, then gathers every
// row under every symmetry and draws one sample into arrays of exactly n rows, and
// compares with what tests/replay_ref.py recorded.  The file: a header line
//   n E H B moves
// per move E lines (meta, the black, white and possible_moves words in hex, skip,
// reward, done, N*N visits); a line with the gather's row count; per gathered row
// a line (row, sym, state, meta, outcome, the 3W words in hex, N*N visits); then
// the sample: augment seed id_key counter count, and per row a line (row, sym,
// outcome).  Test infrastructure only.
#define REPLAY_MAIN
#include <stdio.h>

#include <vector>

#include "replay_host.cpp"

namespace {

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
    int n, E, H, B, moves, cases = 0;
    while (fscanf(f, "%d %d %d %d %d", &n, &E, &H, &B, &moves) == 5) {
        if (bad(n, E, H, B) || moves < 1) return 2;
        const int W = (n * n + 63) / 64, NN = n * n;
        // a workspace of exactly the reported size and of garbage
        std::vector<uint64_t> ws(host_replay_ws_words(n, E, H, B), 0xdeadbeefdeadbeefull);
        if (host_replay_begin(n, E, H, B, ws.data())) return 2;
        std::vector<uint64_t> boards((size_t)E * 2 * W), legal((size_t)E * W);
        std::vector<uint16_t> meta(E);
        std::vector<uint8_t> skip(E), dones(E);
        std::vector<int32_t> rewards(E), visits((size_t)E * NN);
        for (int m = 0; m < moves; ++m) {
            for (int e = 0; e < E; ++e) {
                int mt, sk, rw, dn;
                if (fscanf(f, "%d", &mt) != 1 || !read_hex(f, &boards[(size_t)e * 2 * W], 2 * W) ||
                    !read_hex(f, &legal[(size_t)e * W], W) || fscanf(f, "%d %d %d", &sk, &rw, &dn) != 3)
                    return 2;
                meta[e] = (uint16_t)mt;
                skip[e] = (uint8_t)sk;
                rewards[e] = rw;
                dones[e] = (uint8_t)dn;
                for (int a = 0; a < NN; ++a)
                    if (fscanf(f, "%d", &visits[(size_t)e * NN + a]) != 1) return 2;
            }
            if (host_replay_append(n, E, H, B, ws.data(), boards.data(), meta.data(), legal.data(), visits.data(),
                                   m % 2 ? skip.data() : nullptr))
                return 2;
            if (host_replay_label(n, E, H, B, ws.data(), rewards.data(), dones.data())) return 2;
        }
        int cnt;
        if (fscanf(f, "%d", &cnt) != 1 || cnt < 1 || cnt > B) return 2;
        std::vector<int32_t> rows_in(cnt), want_state(cnt), want_meta(cnt), want_outcome(cnt);
        std::vector<uint8_t> sym_in(cnt);
        std::vector<uint64_t> want_words((size_t)cnt * 3 * W);
        std::vector<int32_t> want_visits((size_t)cnt * NN);
        for (int i = 0; i < cnt; ++i) {
            int s;
            if (fscanf(f, "%d %d %d %d %d", &rows_in[i], &s, &want_state[i], &want_meta[i], &want_outcome[i]) != 5 ||
                !read_hex(f, &want_words[(size_t)i * 3 * W], 3 * W))
                return 2;
            sym_in[i] = (uint8_t)s;
            for (int a = 0; a < NN; ++a)
                if (fscanf(f, "%d", &want_visits[(size_t)i * NN + a]) != 1) return 2;
        }
        {
            // arrays of exactly cnt rows
            std::vector<uint8_t> state(cnt, 7), sym(cnt, 7);
            std::vector<uint64_t> gb((size_t)cnt * 2 * W, 7), gl((size_t)cnt * W, 7);
            std::vector<uint16_t> gm(cnt, 7);
            std::vector<int32_t> gv((size_t)cnt * NN, 7), go(cnt, 7), gr(cnt, 7);
            if (host_replay_batch(n, E, H, B, ws.data(), cnt, rows_in.data(), sym_in.data(), 0, 0, 0, 0, state.data(),
                                  gb.data(), gm.data(), gl.data(), gv.data(), go.data(), gr.data(), sym.data()))
                return 2;
            for (int i = 0; i < cnt; ++i) {
                bool ok = state[i] == want_state[i] && gm[i] == want_meta[i] && go[i] == want_outcome[i] &&
                          sym[i] == (sym_in[i] & 7);
                for (int j = 0; j < 2 * W; ++j) ok = ok && gb[(size_t)i * 2 * W + j] == want_words[(size_t)i * 3 * W + j];
                for (int j = 0; j < W; ++j) ok = ok && gl[(size_t)i * W + j] == want_words[(size_t)i * 3 * W + 2 * W + j];
                for (int a = 0; a < NN; ++a) ok = ok && gv[(size_t)i * NN + a] == want_visits[(size_t)i * NN + a];
                if (!ok) {
                    fprintf(stderr, "FAILED case %d gathered row %d (store row %d, symmetry %d)\n", cases, i, rows_in[i],
                            sym_in[i]);
                    return 1;
                }
            }
            // the same through the staging rows: only the visits are the caller's
            std::vector<int32_t> only((size_t)cnt * NN, 7);
            if (host_replay_batch(n, E, H, B, ws.data(), cnt, rows_in.data(), sym_in.data(), 0, 0, 0, 0, nullptr, nullptr,
                                  nullptr, nullptr, only.data(), nullptr, nullptr, nullptr))
                return 2;
            if (only != want_visits) {
                fprintf(stderr, "FAILED case %d: the visits alone\n", cases);
                return 1;
            }
        }
        int augment, scnt;
        unsigned long long seed, id_key, counter;
        if (fscanf(f, "%d %llu %llu %llu %d", &augment, &seed, &id_key, &counter, &scnt) != 5 || scnt < 1 || scnt > B)
            return 2;
        std::vector<int32_t> srows(scnt, 7), soutcome(scnt, 7);
        std::vector<uint8_t> ssym(scnt, 7);
        if (host_replay_batch(n, E, H, B, ws.data(), scnt, nullptr, nullptr, augment, seed, (uint32_t)id_key, counter,
                              nullptr, nullptr, nullptr, nullptr, nullptr, soutcome.data(), srows.data(), ssym.data()))
            return 2;
        for (int i = 0; i < scnt; ++i) {
            int wr, wsym, wo;
            if (fscanf(f, "%d %d %d", &wr, &wsym, &wo) != 3) return 2;
            if (srows[i] != wr || ssym[i] != wsym || soutcome[i] != wo) {
                fprintf(stderr, "FAILED case %d sample %d: row %d sym %d outcome %d, expected %d %d %d\n", cases, i,
                        srows[i], ssym[i], soutcome[i], wr, wsym, wo);
                return 1;
            }
        }
        int64_t counts[3];
        if (host_replay_counts(n, E, H, B, ws.data(), counts)) return 2;
        if (counts[0] + counts[1] + counts[2] != (int64_t)E * H) return 1;
        ++cases;
    }
    fclose(f);
    if (!cases) return 2;
    printf("replay store under ASan and UBSan: %d cases clean\n", cases);
    return 0;
}
