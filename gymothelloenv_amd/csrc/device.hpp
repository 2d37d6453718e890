// device.hpp -- HIP/CDNA4 device code of the vectorised Othello rules engine,
// for kernels_n.hip (compiled once per board size N, so the templates build in
// parallel): the headers below, one concern each, and the small kernels.
//   state.hpp    a board on the device: meta bits, reset position, Lane, Rng, tallies
//   engines.hpp  the rule engines (Solo / Fills / FillsW / Quartet) and step_lane
//   policy.hpp   MaxiMin and policy_action
//   play.hpp     k_play, k_play_rand, k_play_rand_w
//   vs.hpp       k_reset_vs, k_step_vs
//   observe.hpp  k_observe, k_observe_w, obs_stream, obs_tail
//
// The reference's per-step Python work -- get_possible_actions'
// N*N*8 ray walks (othello.py:313-343), update_board (:391-410), step's
// pass / double-pass / sudden-death / reward logic (:412-462) -- becomes a few
// hundred integer VALU ops per lane.  No MFMA: the work is bit manipulation.
#pragma once
#include "observe.hpp"
#include "play.hpp"
#include "vs.hpp"

namespace oth_dev {

template <int N>
__global__ __launch_bounds__(BLOCK) void k_reset(uint64_t* __restrict__ boards, uint16_t* __restrict__ meta,
                                                 uint64_t* __restrict__ legal, int E,
                                                 const uint8_t* __restrict__ mask, Rng rng, uint64_t ply) {
    ply += *rng.ply_off;  // graph-region offset (oth_graph_end); 0 eagerly
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= E) return;
    if (mask && !mask[e]) return;
    Lane<N> s;
    reset_lane<N>(s, rng.seed, rng.id_base + (uint32_t)e, ply, RNG_OPENING_RESET, rng.init_rand);
    store_lane<N>(s, boards, meta, legal, e);
}

// oth_step: external actions, one ply.
template <int N>
__global__ __launch_bounds__(BLOCK) void k_step(uint64_t* __restrict__ boards, uint16_t* __restrict__ meta,
                                                uint64_t* __restrict__ legal, int E, uint32_t flags,
                                                const int32_t* __restrict__ actions, int32_t* __restrict__ rewards,
                                                uint8_t* __restrict__ dones, unsigned long long* __restrict__ wdl,
                                                Rng rng, uint64_t ply) {
    ply += *rng.ply_off;  // graph-region offset (oth_graph_end); 0 eagerly
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t cb = 0, cd = 0, cw = 0;
    WaveSlot slot(wdl, e, E);
    if (e < E) {
        Lane<N> s;
        load_lane<N>(s, boards, meta, legal, e);
        const int a = actions[e];  // with the board's loads, not behind the terminated test
        const bool was_term = (s.meta & M_TERMINATED) != 0;
        int r, d, win;
        step_lane<N>(s, a, flags, r, d, win, Solo<N>(0, nullptr));
        if (d && !was_term) {
            cb = win == BLACK_DISK;
            cd = win == NO_DISK;
            cw = win == WHITE_DISK;
            if (flags & OTH_AUTO_RESET)
                reset_lane<N>(s, rng.seed, rng.id_base + (uint32_t)e, ply, RNG_OPENING_AUTO, rng.init_rand);
        }
        store_lane<N>(s, boards, meta, legal, e);
        if (rewards) rewards[e] = r;
        if (dones) dones[e] = (uint8_t)d;
    }
    slot.count(cb != 0, cd != 0, cw != 0);
    slot.flush();
}

template <int N>
__global__ __launch_bounds__(BLOCK) void k_legal_moves(const uint64_t* __restrict__ mover,
                                                       const uint64_t* __restrict__ opp, uint64_t* __restrict__ out,
                                                       int n) {
    constexpr int W = Geo<N>::W;
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= n) return;
    BB<W> P, O;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        P.w[i] = mover[(size_t)e * W + i] & Geo<N>::BOARD.w[i];
        O.w[i] = opp[(size_t)e * W + i] & Geo<N>::BOARD.w[i] & ~P.w[i];
    }
    const BB<W> L = legal_moves<N>(P, O);
#pragma unroll
    for (int i = 0; i < W; ++i) out[(size_t)e * W + i] = L.w[i];
}

template <int N, int POLICY>
__global__ __launch_bounds__(BLOCK) void k_policy_actions(const uint64_t* __restrict__ boards,
                                                          const uint16_t* __restrict__ meta,
                                                          const uint64_t* __restrict__ legal, int E,
                                                          int32_t* __restrict__ out, int depth) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= E) return;
    Lane<N> s;
    load_lane<N>(s, boards, meta, legal, e);
    out[e] = policy_action<N, POLICY>(s, Solo<N>(0, nullptr), depth);
}

template <int N>
__global__ __launch_bounds__(BLOCK) void k_set_turn(const uint64_t* __restrict__ boards, uint16_t* __restrict__ meta,
                                                    uint64_t* __restrict__ legal, int E, int turn,
                                                    const uint8_t* __restrict__ mask) {
    constexpr int W = Geo<N>::W;
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= E) return;
    if (mask && !mask[e]) return;
    BB<W> b, w;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        b.w[i] = boards[(size_t)e * 2 * W + i];
        w.w[i] = boards[(size_t)e * 2 * W + W + i];
    }
    const BB<W> L = turn == WHITE_DISK ? legal_moves<N>(w, b) : legal_moves<N>(b, w);
#pragma unroll
    for (int i = 0; i < W; ++i) legal[(size_t)e * W + i] = L.w[i];
    meta[e] = (uint16_t)((meta[e] & ~M_TURN_WHITE) | (turn == WHITE_DISK ? M_TURN_WHITE : 0u));
}

template <int N>
__global__ __launch_bounds__(BLOCK) void k_count(const uint64_t* __restrict__ boards, int E,
                                                 int32_t* __restrict__ out) {
    constexpr int W = Geo<N>::W;
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= E) return;
    int b = 0, w = 0;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        b += popc64(boards[(size_t)e * 2 * W + i]);
        w += popc64(boards[(size_t)e * 2 * W + W + i]);
    }
    out[2 * (size_t)e] = w;
    out[2 * (size_t)e + 1] = b;
}

// oth_step_sync: one board -- the single-board drop-in classes (BASELINE config
// 1) -- stepped with a host action passed by value, then its whole record
// (oth_record: state, reward / done, count_disks, GreedyPolicy's move,
// get_observation and board_state) written into mapped host memory by the same
// launch, the sequence number last behind a system-scope fence, so the host
// can read the record as soon as that number lands.  One wave: every lane
// holds the board (the step is tiny), lane 0 stores the state back, the lanes
// write the squares of the observation planes.
template <int N>
__global__ __launch_bounds__(64) void k_record(uint64_t* __restrict__ boards, uint16_t* __restrict__ meta,
                                               uint64_t* __restrict__ legal, int board, int step, int action,
                                               uint32_t flags, int planes, unsigned long long* __restrict__ wdl,
                                               Rng rng, uint64_t ply, oth_record* __restrict__ rec, uint32_t seq) {
    constexpr int W = Geo<N>::W, NN = N * N;
    static_assert(W <= OTH_RECORD_MAX_WORDS && NN <= OTH_RECORD_MAX_SQUARES, "record capacity");
    ply += *rng.ply_off;
    const int lane = threadIdx.x;
    WaveSlot slot(wdl, board >> 6);
    Lane<N> s;
    load_lane<N>(s, boards, meta, legal, board);
    int r = 0, d = 0, win = NO_DISK;
    bool ended = false;
    if (step & 1) {
        const bool was_term = (s.meta & M_TERMINATED) != 0;
        step_lane<N>(s, action, flags, r, d, win, Solo<N>(0, nullptr));
        ended = d && !was_term;
        if (ended && (flags & OTH_AUTO_RESET))
            reset_lane<N>(s, rng.seed, rng.id_base + (uint32_t)board, ply, RNG_OPENING_AUTO, rng.init_rand);
        if (lane == 0 && !was_term) store_lane<N>(s, boards, meta, legal, board);
    }
    slot.count(lane == 0 && ended && win == BLACK_DISK, lane == 0 && ended && win == NO_DISK,
               lane == 0 && ended && win == WHITE_DISK);
    slot.flush();
    const bool tw = (s.meta & M_TURN_WHITE) != 0;
    const int sign = tw ? 1 : -1;  // othello.py:364-369: mover +1
    for (int a = lane; a < NN; a += 64) {
        const int isb = (int)((s.black.w[a / 64] >> (a % 64)) & 1u), isw = (int)((s.white.w[a / 64] >> (a % 64)) & 1u);
        rec->board_state[a] = (int8_t)(isw - isb);
        rec->obs[a] = (int8_t)((isw - isb) * sign);
        if (planes == 2) rec->obs[NN + a] = (int8_t)((s.legal.w[a / 64] >> (a % 64)) & 1u);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < W; ++i) {
            rec->black[i] = s.black.w[i];
            rec->white[i] = s.white.w[i];
            rec->legal[i] = s.legal.w[i];
        }
        rec->meta = (uint16_t)s.meta;
        rec->done = (uint8_t)d;
        rec->planes = (uint8_t)planes;
        rec->reward = r;
        rec->white_cnt = popcount(s.white);
        rec->black_cnt = popcount(s.black);
        // (one lane's bit-plane flip counts: the bare call 8.96 -> 8.43 us without them, so only on request)
        rec->greedy = !(step & OTH_RECORD_GREEDY) ? OTH_RECORD_NO_GREEDY
                                                  : (popcount(s.legal) ? greedy_action<N>(s, Solo<N>(0, nullptr)) : -1);
    }
    __threadfence_system();  // every lane's record bytes before the sequence number
    __syncthreads();
    if (lane == 0) {
        __threadfence_system();
        *reinterpret_cast<volatile uint32_t*>(&rec->seq) = seq;
    }
}

}  // namespace oth_dev
