// Host build of the replay store (csrc/replay.hpp: replay_append_board,
// replay_label_board, the rank step, replay_emit, replay_transform -- the text the
// device kernels run, compiled with g++) for tests/test_replay_host.py and
// tests/test_replay_symmetry_cpu.py: a shared library with C linkage that has
// oth_replay_begin / _append / _label / _counts / _gather / _sample and
// oth_symmetry_masks on host memory.  tests/host/replay_san_main.cpp includes this
// file under -fsanitize=address,undefined.  Test infrastructure only.
#include <stdint.h>

#include "../../gymothelloenv_amd/csrc/replay.hpp"

using namespace oth;

namespace {

template <int N>
void begin_n(const ReplayWs<N>& ws) {
    ws.put_tags();
    for (uint32_t e = 0; e < ws.E; ++e) replay_begin_board<N>(ws, e);
    for (size_t i = 0; i < (ws.rows() + 7) / 8; ++i) replay_begin_word<N>(ws, i);
}

template <int N>
void append_n(const ReplayWs<N>& ws, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal,
              const int32_t* visits, const uint8_t* skip) {
    constexpr int W = Geo<N>::W;
    if (!ws.begun()) return;
    for (uint32_t e = 0; e < ws.E; ++e)
        replay_append_board<N>(ws, e, boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W, legal + (size_t)e * W,
                               meta[e], visits + (size_t)e * N * N, skip && skip[e] != 0);
}

template <int N>
void label_n(const ReplayWs<N>& ws, const int32_t* rewards, const uint8_t* dones) {
    if (!ws.begun()) return;
    for (uint32_t e = 0; e < ws.E; ++e) replay_label_board<N>(ws, e, rewards[e], dones[e] != 0);
}

// the rank step's two launches
template <int N>
void rank_n(const ReplayWs<N>& ws, int64_t* counts) {
    if (!ws.begun()) return;
    for (size_t c = 0; c < ws.chunks(); ++c) replay_count_chunk<N>(ws, c);
    replay_scan<N>(ws, counts);
}

// rows_in null: the sample's draw
template <int N>
void batch_n(const ReplayWs<N>& ws, int n, const int32_t* rows_in, const uint8_t* sym_in, bool augment, uint64_t seed,
             uint32_t id_key, uint64_t counter, const ReplayBatch& out) {
    if (!ws.begun()) return;
    if (!rows_in) rank_n<N>(ws, nullptr);
    uint64_t* boards = out.boards ? out.boards : ws.stage_boards();
    uint16_t* meta = out.meta ? out.meta : ws.stage_meta();
    uint64_t* legal = out.legal ? out.legal : ws.stage_legal();
    for (int i = 0; i < n; ++i) {
        long long row;
        int s;
        if (rows_in) {
            row = rows_in[i];
            s = sym_in ? sym_in[i] & 7 : 0;
        } else {
            row = replay_draw<N>(ws, (uint32_t)i, augment, seed, id_key, counter, s);
        }
        replay_emit<N>(ws, (size_t)i, row, s, out, boards, meta, legal);
    }
}

template <int N>
void masks_n(int n, int planes, const uint8_t* sym, const uint64_t* in, uint64_t* out) {
    constexpr int W = Geo<N>::W;
    for (long long t = 0; t < (long long)n * planes; ++t)
        replay_transform<N, 1>(in + (size_t)t * W, sym[t / planes] & 7, out + (size_t)t * W);
}

bool bad(int n, int E, int H, int B) {
    return n < 4 || n > 16 || E < 1 || H < 1 || H > REPLAY_MAX_HORIZON || B < 1 || B > REPLAY_MAX_BATCH ||
           (uint64_t)E * (uint64_t)H > (uint64_t)REPLAY_MAX_ROWS;
}

}  // namespace

#ifdef REPLAY_MAIN  // the sanitizer program's size only, a shorter build
#define SIZES(X) X(6)
#else
#define SIZES(X) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
#endif
#define WS(S) ReplayWs<S>{ws, (uint32_t)E, (uint32_t)H, (uint32_t)B}

extern "C" uint64_t host_replay_ws_words(int n, int E, int H, int B) {
    return replay_ws_words(n, (uint64_t)E, (uint64_t)H, (uint64_t)B);
}

extern "C" int host_replay_sigma(int n, int s, int a) {
    switch (n) {
#define CASE(S) \
    case S: return replay_sigma<S>(s, a);
        SIZES(CASE)
#undef CASE
        default: return -1;
    }
}

extern "C" int host_replay_begin(int n, int E, int H, int B, uint64_t* ws) {
    if (bad(n, E, H, B)) return -1;
    switch (n) {
#define CASE(S) \
    case S: begin_n<S>(WS(S)); break;
        SIZES(CASE)
#undef CASE
        default: return -1;
    }
    return 0;
}

extern "C" int host_replay_append(int n, int E, int H, int B, uint64_t* ws, const uint64_t* boards, const uint16_t* meta,
                                  const uint64_t* legal, const int32_t* visits, const uint8_t* skip) {
    if (bad(n, E, H, B) || !visits) return -1;
    switch (n) {
#define CASE(S) \
    case S: append_n<S>(WS(S), boards, meta, legal, visits, skip); break;
        SIZES(CASE)
#undef CASE
        default: return -1;
    }
    return 0;
}

extern "C" int host_replay_label(int n, int E, int H, int B, uint64_t* ws, const int32_t* rewards,
                                 const uint8_t* dones) {
    if (bad(n, E, H, B) || !rewards || !dones) return -1;
    switch (n) {
#define CASE(S) \
    case S: label_n<S>(WS(S), rewards, dones); break;
        SIZES(CASE)
#undef CASE
        default: return -1;
    }
    return 0;
}

extern "C" int host_replay_counts(int n, int E, int H, int B, uint64_t* ws, int64_t* out) {
    if (bad(n, E, H, B) || !out) return -1;
    switch (n) {
#define CASE(S) \
    case S: rank_n<S>(WS(S), out); break;
        SIZES(CASE)
#undef CASE
        default: return -1;
    }
    return 0;
}

// oth_replay_gather (rows_in given) and oth_replay_sample (rows_in NULL)
extern "C" int host_replay_batch(int n, int E, int H, int B, uint64_t* ws, int cnt, const int32_t* rows_in,
                                 const uint8_t* sym_in, int augment, uint64_t seed, uint32_t id_key, uint64_t counter,
                                 uint8_t* state, uint64_t* boards, uint16_t* meta, uint64_t* legal, int32_t* visits,
                                 int32_t* outcome, int32_t* rows, uint8_t* sym) {
    if (bad(n, E, H, B) || cnt < 1 || cnt > B) return -1;
    const ReplayBatch out{state, boards, meta, legal, visits, outcome, rows, sym};
    switch (n) {
#define CASE(S) \
    case S: batch_n<S>(WS(S), cnt, rows_in, sym_in, augment != 0, seed, id_key, counter, out); break;
        SIZES(CASE)
#undef CASE
        default: return -1;
    }
    return 0;
}

extern "C" int host_symmetry_masks(int n, int cnt, int planes, const uint8_t* sym, const uint64_t* in, uint64_t* out) {
    if (cnt < 1 || planes < 1 || !sym || !in || !out || in == out) return -1;
    switch (n) {
#define CASE(S) \
    case S: masks_n<S>(cnt, planes, sym, in, out); break;
        SIZES(CASE)
#undef CASE
        default: return -1;
    }
    return 0;
}
