// replay.hpp -- oth_replay_begin / _append / _label / _counts / _gather / _sample
// and oth_symmetry_masks: the self-play samples (position, visit target, outcome
// from the mover's side) kept in a ring of H record slots per board, labelled
// when the game ends and drawn as minibatches under the eight symmetries of the
// board (the spec is the header's comment on oth_replay_begin: every output is
// an integer function of the inputs).
//
// The workspace, in 64-bit words (ReplayWs; E boards, H slots a board, R = E H
// rows, row e H + j = slot j of board e, C = ceil(R / 1024) chunks, B rows of
// staging):
//   [0], [1]              the tags of the store that began here (replay_tag0 / _tag1)
//   [2, 2 + 2E)           a board's header: count, then span | last_turn << 32
//   then ceil(R / 8)      the rows' state bytes: state | turn << 7 (the padding
//                         bytes of the last word are zero from begin on)
//   then ceil(R / 2)      the rows' outcomes, int32
//   then C                a chunk's rows in state OPEN | LABELLED << 32
//   then ceil((C + 1) / 2)  the exclusive prefix of the chunks' LABELLED counts, uint32 [C + 1]
//   then ceil(B / 4), [B][2W], [B][W]   a batch's meta, boards and moves in exchange format where the
//                         caller gave no array of its own: the observation kernels read these
//   then [R][3W]          the rows' black, white and stored possible_moves
//   then ceil(R NN / 2)   the rows' cleaned visits, int32 [R][NN]
// It holds counts and positions only, no address: a byte copy is a checkpoint.
//
// The part outside __HIPCC__ is plain host/device code over bitboard.hpp, which
// tests/host/replay_host.cpp compiles with g++ and loops over boards and rows.
//
// Device mapping: append and label are a lane per board
// (every word of a board's header and of its H rows is written by that lane
// alone); a batch is a lane per sample.  The rank-to-row step of a sample is
// free of atomics: a block per chunk counts its states, one workgroup scans the
// chunk counts, and each sample binary-searches the prefix and walks one chunk's
// state bytes.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>

#include "bitboard.hpp"

namespace oth {

constexpr int REPLAY_EMPTY = 0, REPLAY_OPEN = 1, REPLAY_LABELLED = 2;
constexpr int REPLAY_MAX_HORIZON = 65536, REPLAY_MAX_ROWS = 1 << 24, REPLAY_MAX_BATCH = 1 << 20;
constexpr int REPLAY_VISITS_MAX = (1 << 24) - 1, REPLAY_OUTCOME_MAX = 32768;
constexpr int REPLAY_CHUNK = 1024;          // rows a chunk of the rank step
constexpr uint32_t REPLAY_RNG_SAMPLE = 5u;  // Philox purpose word of oth_replay_sample's draw (state.hpp RNG_REPLAY_SAMPLE)
constexpr uint32_t REPLAY_F_TURN = 0x80u;   // a state byte's turn bit

constexpr uint64_t replay_chunks(uint64_t R) { return (R + REPLAY_CHUNK - 1) / REPLAY_CHUNK; }
// the words of the workspace in front of the rows' discs, and of the whole workspace
constexpr uint64_t replay_head_words(int n, uint64_t E, uint64_t H, uint64_t B) {
    return 2u + 2u * E + (E * H + 7u) / 8u + (E * H + 1u) / 2u + replay_chunks(E * H) +
           (replay_chunks(E * H) + 2u) / 2u + (B + 3u) / 4u + 3u * (uint64_t)((n * n + 63) / 64) * B;
}
constexpr uint64_t replay_ws_words(int n, uint64_t E, uint64_t H, uint64_t B) {
    return replay_head_words(n, E, H, B) + 3u * (uint64_t)((n * n + 63) / 64) * E * H +
           (E * H * (uint64_t)(n * n) + 1u) / 2u;
}
OTH_HD uint64_t replay_tag0(int n, uint32_t E) {
    return 0x7265706c00000000ull ^ ((uint64_t)(uint32_t)n << 56) ^ (uint64_t)E;
}
OTH_HD uint64_t replay_tag1(uint32_t H, uint32_t B) { return 0x6179000000000000ull ^ ((uint64_t)H << 24) ^ (uint64_t)B; }

template <int N>
struct ReplayWs {
    static constexpr int W = Geo<N>::W, NN = N * N;
    uint64_t* base;
    uint32_t E, H, B;
    OTH_HD size_t rows() const { return (size_t)E * H; }
    OTH_HD size_t chunks() const { return (rows() + REPLAY_CHUNK - 1) / REPLAY_CHUNK; }
    OTH_HD uint64_t* hdr(uint32_t e) const { return base + 2 + 2 * (size_t)e; }
    OTH_HD uint64_t* state_words() const { return base + 2 + 2 * (size_t)E; }
    OTH_HD uint8_t* state() const { return reinterpret_cast<uint8_t*>(state_words()); }
    OTH_HD int32_t* outcome() const { return reinterpret_cast<int32_t*>(state_words() + (rows() + 7) / 8); }
    OTH_HD uint64_t* chunk_counts() const { return state_words() + (rows() + 7) / 8 + (rows() + 1) / 2; }
    OTH_HD uint32_t* prefix() const { return reinterpret_cast<uint32_t*>(chunk_counts() + chunks()); }
    OTH_HD uint16_t* stage_meta() const { return reinterpret_cast<uint16_t*>(chunk_counts() + chunks() + (chunks() + 2) / 2); }
    OTH_HD uint64_t* stage_boards() const { return chunk_counts() + chunks() + (chunks() + 2) / 2 + ((size_t)B + 3) / 4; }
    OTH_HD uint64_t* stage_legal() const { return stage_boards() + 2 * W * (size_t)B; }
    OTH_HD uint64_t* discs(size_t row) const { return stage_legal() + W * (size_t)B + row * 3 * W; }
    OTH_HD int32_t* visits(size_t row) const {
        return reinterpret_cast<int32_t*>(stage_legal() + W * (size_t)B + rows() * 3 * W) + row * NN;
    }
    OTH_HD void put_tags() const {
        base[0] = replay_tag0(N, E);
        base[1] = replay_tag1(H, B);
    }
    // a begin of this geometry wrote the workspace
    OTH_HD bool begun() const { return base[0] == replay_tag0(N, E) && base[1] == replay_tag1(H, B); }
};

// the caller's arrays of one batch (oth_replay_batch without the observation), each may be null
struct ReplayBatch {
    uint8_t* state;
    uint64_t* boards;
    uint16_t* meta;
    uint64_t* legal;
    int32_t* visits;
    int32_t* outcome;
    int32_t* rows;
    uint8_t* sym;
};

// sigma_s(a): the square that stored square a goes to under symmetry s (transpose, then the row flip, then
// the column flip)
template <int N>
OTH_HD int replay_sigma(int s, int a) {
    const int r = a / N, c = a % N;
    const int r1 = (s & 1) ? c : r, c1 = (s & 1) ? r : c;
    const int r2 = (s & 2) ? N - 1 - r1 : r1, c2 = (s & 4) ? N - 1 - c1 : c1;
    return r2 * N + c2;
}

// P planes of W words under symmetry s: bit sigma_s(a) of out is bit a of in, squares off the board dropped
template <int N, int P>
OTH_HD void replay_transform(const uint64_t* in, int s, uint64_t* out) {
    constexpr int W = Geo<N>::W, NN = N * N;
    BB<W> src[P], dst[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int j = 0; j < W; ++j) src[p].w[j] = in[p * W + j];
        dst[p] = zero<W>();
    }
    for (int a = 0; a < NN; ++a) {
        const BB<W> to = square<W>(replay_sigma<N>(s, a));
#pragma unroll
        for (int p = 0; p < P; ++p) dst[p] |= select_if(test(src[p], a), to);
    }
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < W; ++j) out[p * W + j] = dst[p].w[j];
}

// oth_replay_begin: the header of board e, and word i of the state bytes (the last word's padding included)
template <int N>
OTH_HD void replay_begin_board(const ReplayWs<N>& ws, uint32_t e) {
    ws.hdr(e)[0] = 0ull;
    ws.hdr(e)[1] = 0ull;
}
template <int N>
OTH_HD void replay_begin_word(const ReplayWs<N>& ws, size_t i) {
    ws.state_words()[i] = 0ull;
}

// oth_replay_append for board e (the handle's black, white, stored possible_moves and meta; visits: the
// board's N*N)
template <int N>
OTH_HD void replay_append_board(const ReplayWs<N>& ws, uint32_t e, const uint64_t* black, const uint64_t* white,
                                const uint64_t* stored, uint32_t meta, const int32_t* visits, bool skip) {
    constexpr int W = Geo<N>::W, NN = N * N;
    uint64_t* h = ws.hdr(e);
    const uint32_t turn = meta & 1u;
    uint32_t span = (uint32_t)h[1];
    h[1] = (uint64_t)span | (uint64_t)turn << 32;
    if ((meta & 2u) || skip) return;
    BB<W> Lg;
#pragma unroll
    for (int j = 0; j < W; ++j) Lg.w[j] = stored[j];
    Lg = Lg & Geo<N>::BOARD;
    uint64_t sum = 0;
    for (int a = 0; a < NN; ++a) {
        const int32_t v = visits[a];
        if (test(Lg, a) && v > 0) sum += (uint64_t)(v > REPLAY_VISITS_MAX ? REPLAY_VISITS_MAX : v);
    }
    if (sum == 0) return;
    const uint64_t count = h[0];
    const size_t row = (size_t)e * ws.H + (size_t)(count % ws.H);
    uint64_t* d = ws.discs(row);
#pragma unroll
    for (int j = 0; j < W; ++j) {
        d[j] = black[j];
        d[W + j] = white[j];
        d[2 * W + j] = stored[j];
    }
    int32_t* c = ws.visits(row);
    for (int a = 0; a < NN; ++a) {
        const int32_t v = visits[a];
        c[a] = test(Lg, a) && v > 0 ? (v > REPLAY_VISITS_MAX ? REPLAY_VISITS_MAX : v) : 0;
    }
    ws.state()[row] = (uint8_t)(REPLAY_OPEN | (turn ? REPLAY_F_TURN : 0u));
    ws.outcome()[row] = 0;
    h[0] = count + 1;
    span = span < ws.H ? span + 1 : ws.H;
    h[1] = (uint64_t)span | (uint64_t)turn << 32;
}

// oth_replay_label for board e
template <int N>
OTH_HD void replay_label_board(const ReplayWs<N>& ws, uint32_t e, int32_t reward, bool done) {
    if (!done) return;
    uint64_t* h = ws.hdr(e);
    const int32_t z = reward < -REPLAY_OUTCOME_MAX ? -REPLAY_OUTCOME_MAX
                                                   : (reward > REPLAY_OUTCOME_MAX ? REPLAY_OUTCOME_MAX : reward);
    const uint64_t count = h[0];
    uint32_t span = (uint32_t)h[1];
    const uint32_t last_turn = (uint32_t)(h[1] >> 32) & 1u;
    if (span > ws.H) span = ws.H;  // (a header no begin wrote: nothing outside the board's rows is followed)
    for (uint32_t k = 0; k < span && (uint64_t)k < count; ++k) {
        const size_t row = (size_t)e * ws.H + (size_t)((count - 1 - k) % ws.H);
        const uint32_t st = ws.state()[row];
        if ((st & 3u) != (uint32_t)REPLAY_OPEN) continue;
        ws.state()[row] = (uint8_t)((st & ~3u) | (uint32_t)REPLAY_LABELLED);
        ws.outcome()[row] = ((st & REPLAY_F_TURN) != 0) == (last_turn != 0) ? z : -z;
    }
    h[1] = (uint64_t)last_turn << 32;
}

// the rank step, one chunk: its rows in state OPEN and LABELLED (the device counts a chunk on a block)
template <int N>
OTH_HD void replay_count_chunk(const ReplayWs<N>& ws, size_t c) {
    const size_t lo = c * REPLAY_CHUNK, R = ws.rows();
    const size_t hi = lo + REPLAY_CHUNK < R ? lo + REPLAY_CHUNK : R;
    uint32_t open = 0, lab = 0;
    for (size_t i = lo; i < hi; ++i) {
        const uint32_t st = ws.state()[i] & 3u;
        open += st == (uint32_t)REPLAY_OPEN;
        lab += st == (uint32_t)REPLAY_LABELLED;
    }
    ws.chunk_counts()[c] = (uint64_t)open | (uint64_t)lab << 32;
}

// ... the scan of the chunk counts (the device scans on one workgroup); counts: EMPTY, OPEN, LABELLED rows, or null
template <int N>
OTH_HD void replay_scan(const ReplayWs<N>& ws, int64_t* counts) {
    uint32_t* pre = ws.prefix();
    uint64_t open = 0, lab = 0;
    const size_t C = ws.chunks();
    for (size_t c = 0; c < C; ++c) {
        pre[c] = (uint32_t)lab;
        open += (uint32_t)ws.chunk_counts()[c];
        lab += ws.chunk_counts()[c] >> 32;
    }
    pre[C] = (uint32_t)lab;
    if (counts) {
        counts[0] = (int64_t)(ws.rows() - open - lab);
        counts[1] = (int64_t)open;
        counts[2] = (int64_t)lab;
    }
}

// ... and the (r + 1)-th LABELLED row in ascending row number, r < M = prefix[C]
template <int N>
OTH_HD long long replay_rank_row(const ReplayWs<N>& ws, uint32_t r) {
    const uint32_t* pre = ws.prefix();
    size_t lo = 0, hi = ws.chunks();  // the chunk c with pre[c] <= r < pre[c + 1]
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) / 2;
        if (pre[mid] <= r) lo = mid;
        else hi = mid;
    }
    uint32_t k = r - pre[lo];
    const size_t w0 = lo * (REPLAY_CHUNK / 8), R = ws.rows();
    const size_t w1 = w0 + REPLAY_CHUNK / 8 < (R + 7) / 8 ? w0 + REPLAY_CHUNK / 8 : (R + 7) / 8;
    for (size_t i = w0; i < w1; ++i) {
        const uint64_t w = ws.state_words()[i];
        uint64_t m = (w >> 1) & ~w & 0x0101010101010101ull;  // a byte's bit 0: state LABELLED (2)
        const uint32_t cnt = (uint32_t)popc64(m);
        if (k >= cnt) {
            k -= cnt;
            continue;
        }
        for (; k > 0; --k) m &= m - 1;
        return (long long)(i * 8 + (size_t)(ctz64(m) >> 3));
    }
    return -1;  // (a prefix that the states no longer match: the EMPTY row)
}

// Row i of a batch: store row `row` (outside [0, R): the EMPTY row) under symmetry s.  boards / meta / legal:
// where the row's exchange format goes (the caller's arrays or the staging area), never null.
template <int N>
OTH_HD void replay_emit(const ReplayWs<N>& ws, size_t i, long long row, int s, const ReplayBatch& out,
                        uint64_t* boards, uint16_t* meta, uint64_t* legal) {
    constexpr int W = Geo<N>::W, NN = N * N;
    const bool in_range = row >= 0 && (unsigned long long)row < (unsigned long long)ws.rows();
    const uint32_t sb = in_range ? ws.state()[row] : 0u;
    const uint32_t st = sb & 3u;
    const bool live = st == (uint32_t)REPLAY_OPEN || st == (uint32_t)REPLAY_LABELLED;
    uint64_t t[3 * W];
    if (live) {
        replay_transform<N, 3>(ws.discs((size_t)row), s, t);
    } else {
#pragma unroll
        for (int j = 0; j < 3 * W; ++j) t[j] = 0ull;
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
        boards[i * 2 * W + j] = t[j];
        boards[i * 2 * W + W + j] = t[W + j];
        legal[i * W + j] = t[2 * W + j];
    }
    meta[i] = (uint16_t)(live && (sb & REPLAY_F_TURN) ? 1u : 0u);
    if (out.state) out.state[i] = (uint8_t)(live ? st : 0u);
    if (out.outcome) out.outcome[i] = live ? ws.outcome()[row] : 0;
    if (out.rows) out.rows[i] = in_range ? (int32_t)row : -1;
    if (out.sym) out.sym[i] = (uint8_t)s;
    if (out.visits) {
        int32_t* v = out.visits + i * NN;
        if (live) {
            const int32_t* c = ws.visits((size_t)row);
            for (int a = 0; a < NN; ++a) v[replay_sigma<N>(s, a)] = c[a];
        } else {
            for (int a = 0; a < NN; ++a) v[a] = 0;
        }
    }
}

// oth_replay_sample's draw of row i: the store row (or -1 for M = 0) and the symmetry
template <int N>
OTH_HD long long replay_draw(const ReplayWs<N>& ws, uint32_t i, bool augment, uint64_t seed, uint32_t id_key,
                             uint64_t counter, int& s) {
    const U4 u = philox4(seed, id_key + i, counter, REPLAY_RNG_SAMPLE);
    s = augment ? (int)(u.y >> 29) : 0;
    const uint32_t M = ws.prefix()[ws.chunks()];
    if (M == 0) return -1;
    return replay_rank_row<N>(ws, (uint32_t)(((uint64_t)u.x * M) >> 32));
}

}  // namespace oth

#if defined(__HIPCC__)
#include "state.hpp"

namespace oth_dev {

static_assert(REPLAY_EMPTY == OTH_REPLAY_EMPTY && REPLAY_OPEN == OTH_REPLAY_OPEN &&
                  REPLAY_LABELLED == OTH_REPLAY_LABELLED && REPLAY_MAX_HORIZON == OTH_REPLAY_MAX_HORIZON &&
                  REPLAY_MAX_ROWS == OTH_REPLAY_MAX_ROWS && REPLAY_MAX_BATCH == OTH_REPLAY_MAX_BATCH,
              "the header's states and limits");
static_assert(REPLAY_RNG_SAMPLE == RNG_REPLAY_SAMPLE, "state.hpp's purpose word");

constexpr int REPLAY_BLOCK = 64;        // one wave a block: a lane per board, or per sample
constexpr int REPLAY_COUNT_BLOCK = 256;  // a block per chunk: four state bytes a lane
constexpr int REPLAY_SCAN_BLOCK = 1024;  // the one workgroup of the scan

// every state word, every board's header, the tags
template <int N>
__global__ __launch_bounds__(256) void k_replay_begin(int E, uint32_t H, uint32_t B, uint64_t* __restrict__ wsp) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const ReplayWs<N> ws{wsp, (uint32_t)E, H, B};
    if (i == 0) ws.put_tags();
    if (i < (size_t)E) replay_begin_board<N>(ws, (uint32_t)i);
    if (i < (ws.rows() + 7) / 8) replay_begin_word<N>(ws, i);
}

// (a workspace whose tags are not this store's -- no begin of this geometry -- is left alone)
template <int N>
__global__ __launch_bounds__(REPLAY_BLOCK) void k_replay_append(const uint64_t* __restrict__ boards,
                                                                const uint16_t* __restrict__ meta,
                                                                const uint64_t* __restrict__ legal, int E, uint32_t H,
                                                                uint32_t B, uint64_t* __restrict__ wsp,
                                                                const int32_t* __restrict__ visits,
                                                                const uint8_t* __restrict__ skip) {
    constexpr int W = Geo<N>::W;
    const long long e = (long long)blockIdx.x * REPLAY_BLOCK + threadIdx.x;
    const ReplayWs<N> ws{wsp, (uint32_t)E, H, B};
    if (e >= E || !ws.begun()) return;
    replay_append_board<N>(ws, (uint32_t)e, boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W,
                           legal + (size_t)e * W, meta[e], visits + (size_t)e * (N * N), skip && skip[e] != 0);
}

template <int N>
__global__ __launch_bounds__(REPLAY_BLOCK) void k_replay_label(int E, uint32_t H, uint32_t B,
                                                               uint64_t* __restrict__ wsp,
                                                               const int32_t* __restrict__ rewards,
                                                               const uint8_t* __restrict__ dones) {
    const long long e = (long long)blockIdx.x * REPLAY_BLOCK + threadIdx.x;
    const ReplayWs<N> ws{wsp, (uint32_t)E, H, B};
    if (e >= E || !ws.begun()) return;
    replay_label_board<N>(ws, (uint32_t)e, rewards[e], dones[e] != 0);
}

// the rank step's first launch: a block per chunk, its OPEN and LABELLED rows summed through the LDS in a
// fixed order
template <int N>
__global__ __launch_bounds__(REPLAY_COUNT_BLOCK) void k_replay_count(int E, uint32_t H, uint32_t B,
                                                                     uint64_t* __restrict__ wsp) {
    __shared__ uint32_t acc[REPLAY_COUNT_BLOCK][2];
    const ReplayWs<N> ws{wsp, (uint32_t)E, H, B};
    if (!ws.begun()) return;
    const size_t c = blockIdx.x, R = ws.rows();
    uint32_t open = 0, lab = 0;
#pragma unroll
    for (int k = 0; k < REPLAY_CHUNK / REPLAY_COUNT_BLOCK; ++k) {
        const size_t i = c * REPLAY_CHUNK + (size_t)threadIdx.x * (REPLAY_CHUNK / REPLAY_COUNT_BLOCK) + k;
        if (i < R) {
            const uint32_t st = ws.state()[i] & 3u;
            open += st == (uint32_t)REPLAY_OPEN;
            lab += st == (uint32_t)REPLAY_LABELLED;
        }
    }
    acc[threadIdx.x][0] = open;
    acc[threadIdx.x][1] = lab;
    __syncthreads();
    for (int s = REPLAY_COUNT_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            acc[threadIdx.x][0] += acc[threadIdx.x + s][0];
            acc[threadIdx.x][1] += acc[threadIdx.x + s][1];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) ws.chunk_counts()[c] = (uint64_t)acc[0][0] | (uint64_t)acc[0][1] << 32;
}

// ... its second: one workgroup, a run of consecutive chunks a lane (at most 2^24 / 1024 / 1024 = 16), the
// lanes' sums scanned through the LDS.  counts: oth_replay_counts' out, or null.
template <int N>
__global__ __launch_bounds__(REPLAY_SCAN_BLOCK) void k_replay_scan(int E, uint32_t H, uint32_t B,
                                                                   uint64_t* __restrict__ wsp,
                                                                   int64_t* __restrict__ counts) {
    __shared__ uint32_t lab_s[REPLAY_SCAN_BLOCK], open_s[REPLAY_SCAN_BLOCK];
    const ReplayWs<N> ws{wsp, (uint32_t)E, H, B};
    if (!ws.begun()) return;
    const size_t C = ws.chunks(), per = (C + REPLAY_SCAN_BLOCK - 1) / REPLAY_SCAN_BLOCK;
    const size_t lo = (size_t)threadIdx.x * per, hi = lo + per < C ? lo + per : C;
    uint32_t open = 0, lab = 0;
    for (size_t c = lo; c < hi; ++c) {
        open += (uint32_t)ws.chunk_counts()[c];
        lab += (uint32_t)(ws.chunk_counts()[c] >> 32);
    }
    lab_s[threadIdx.x] = lab;
    open_s[threadIdx.x] = open;
    __syncthreads();
    for (int d = 1; d < REPLAY_SCAN_BLOCK; d <<= 1) {  // inclusive scan
        const uint32_t a = (int)threadIdx.x >= d ? lab_s[threadIdx.x - d] : 0u;
        const uint32_t b = (int)threadIdx.x >= d ? open_s[threadIdx.x - d] : 0u;
        __syncthreads();
        lab_s[threadIdx.x] += a;
        open_s[threadIdx.x] += b;
        __syncthreads();
    }
    uint32_t run = lab_s[threadIdx.x] - lab;  // the LABELLED rows in front of this lane's chunks
    uint32_t* pre = ws.prefix();
    for (size_t c = lo; c < hi; ++c) {
        pre[c] = run;
        run += (uint32_t)(ws.chunk_counts()[c] >> 32);
    }
    if (threadIdx.x == REPLAY_SCAN_BLOCK - 1) {
        const uint32_t M = lab_s[REPLAY_SCAN_BLOCK - 1], O = open_s[REPLAY_SCAN_BLOCK - 1];
        pre[C] = M;
        if (counts) {
            counts[0] = (int64_t)(ws.rows() - O - M);
            counts[1] = (int64_t)O;
            counts[2] = (int64_t)M;
        }
    }
}

// a batch, a lane per row: oth_replay_gather (rows_in, sym_in) or oth_replay_sample (rows_in null: the draw)
template <int N>
__global__ __launch_bounds__(REPLAY_BLOCK) void k_replay_batch(int E, uint32_t H, uint32_t B,
                                                               uint64_t* __restrict__ wsp, int n,
                                                               const int32_t* __restrict__ rows_in,
                                                               const uint8_t* __restrict__ sym_in, int augment,
                                                               uint64_t seed, uint32_t id_key, uint64_t counter,
                                                               ReplayBatch out, uint64_t* __restrict__ boards,
                                                               uint16_t* __restrict__ meta,
                                                               uint64_t* __restrict__ legal) {
    const long long i = (long long)blockIdx.x * REPLAY_BLOCK + threadIdx.x;
    const ReplayWs<N> ws{wsp, (uint32_t)E, H, B};
    if (i >= n || !ws.begun()) return;
    long long row;
    int s;
    if (rows_in) {
        row = rows_in[i];
        s = sym_in ? sym_in[i] & 7 : 0;
    } else {
        row = replay_draw<N>(ws, (uint32_t)i, augment != 0, seed, id_key, counter, s);
    }
    replay_emit<N>(ws, (size_t)i, row, s, out, boards, meta, legal);
}

// oth_symmetry_masks: a lane per (row, plane)
template <int N>
__global__ __launch_bounds__(256) void k_symmetry_masks(long long total, int planes, const uint8_t* __restrict__ sym,
                                                        const uint64_t* __restrict__ in, uint64_t* __restrict__ out) {
    constexpr int W = Geo<N>::W;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    uint64_t r[W];
    replay_transform<N, 1>(in + (size_t)t * W, sym[t / planes] & 7, r);
#pragma unroll
    for (int j = 0; j < W; ++j) out[(size_t)t * W + j] = r[j];
}

}  // namespace oth_dev
#endif
