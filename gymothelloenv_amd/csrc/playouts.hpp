// playouts.hpp -- oth_playouts: Monte-Carlo playouts from the handle's live
// positions, per board (OTH_PLAYOUT_ROOT) or per legal move (OTH_PLAYOUT_MOVES).
// Nothing of the handle is written: every lane plays a private copy of its
// board, held in registers, to the end of the game and adds the outcome to
// integer counters in LDS; the block stores (or, where a board's playouts are
// split over blocks, atomically adds) each output element once at its end.
//
// Work mapping.  A block serves one group of EPB
// consecutive boards; B blocks share a group, block c of them taking the
// group's tasks c*256 + tid, then + B*256, ...
//   ROOT:  task t of a group is (board t / R, playout t % R).  R < 256 packs
//          EPB = 256 / R boards into a block (65,536 boards at R = 8: every
//          lane plays); R >= 256 gives a board a block, or B of them.
//   MOVES: EPB = 1; task t is (the (t / R)-th set bit of possible_moves,
//          playout t % R) for t < popcount(possible_moves) * R: lanes exist
//          for legal squares only.
// The Philox id of a playout is a function of (global env id, square, r)
// alone, so none of this shows in the results.
#pragma once
#include "engines.hpp"

namespace oth_dev {

constexpr int PLAYOUT_SLOTS = 256;      // LDS counter rows: boards of a ROOT group, squares of a MOVES board
constexpr int PLAYOUT_MAX_PLIES = 256;  // > N*N - 4 + 1: every ply after the first places a disc

// the play engine per board size: flips from the legal scan's fills and rays
// (shifted constants on one-word boards, an LDS ray table on two-word boards,
// where it leaves room for the counters), Kogge-Stone flips without tables for
// three and four words
template <int N>
using PlayoutEng = std::conditional_t<Geo<N>::W == 1, Fills<N>, std::conditional_t<Geo<N>::W == 2, FillsW<N>, Solo<N>>>;

struct PlayoutKey {
    uint64_t seed;
    uint64_t block0;   // Philox block of playout ply 0: counter * 256 / 4
    uint32_t id_key;   // the caller's id offset
    uint32_t id_base;  // the handle's env_id_base
};

template <int N, int MODE>
__global__ __launch_bounds__(BLOCK) void k_playouts(const uint64_t* __restrict__ boards,
                                                    const uint16_t* __restrict__ meta,
                                                    const uint64_t* __restrict__ legal, int E, int R, int EPB, int B,
                                                    PlayoutKey key, int32_t* __restrict__ wdl,
                                                    int32_t* __restrict__ score, int split,
                                                    const uint64_t* __restrict__ tables) {
    using Eng = PlayoutEng<N>;
    constexpr int W = Geo<N>::W, NN = N * N;
    static_assert(BLOCK == 256 && NN <= PLAYOUT_SLOTS, "one counter row per square, one sel8 word a thread");
    __shared__ __attribute__((aligned(16))) uint64_t lds_rays[Eng::RAY_WORDS > 0 ? Eng::RAY_WORDS : 1];
    __shared__ __attribute__((aligned(16))) uint64_t lds_sel[256];
    __shared__ int cnt[PLAYOUT_SLOTS * 4];  // per row {wins, draws, losses, score}
    const uint8_t* sel8 = reinterpret_cast<const uint8_t*>(lds_sel);
    const int tid = threadIdx.x;
    for (int i = tid; i < PLAYOUT_SLOTS * 4; i += BLOCK) cnt[i] = 0;
    if constexpr (W == 1) {  // the handle's sel8 table (k_fill_rays), as k_play_rand
        lds_sel[tid] = tables[SEL8_AT + tid];
        __syncthreads();
    } else if constexpr (W == 2) {
        lds_sel[tid] = sel8_word((uint32_t)tid);
        FillsW<N>::fill(lds_rays);  // (its barrier covers lds_sel and cnt)
    } else {
        __syncthreads();
    }
    const int grp = blockIdx.x / B, chunk = blockIdx.x - grp * B;
    const int e0 = grp * EPB;
    const int ne = min(EPB, E - e0);
    // the group's task count; MOVES: the board's stored possible_moves, none when it is terminated
    BB<W> root_moves;
    int limit;
    if constexpr (MODE == OTH_PLAYOUT_MOVES) {
#pragma unroll
        for (int i = 0; i < W; ++i) root_moves.w[i] = legal[(size_t)e0 * W + i];
        const bool term = (meta[e0] & M_TERMINATED) != 0;
        limit = term ? 0 : popcount(root_moves) * R;
    } else {
        limit = ne * R;
    }
    const uint32_t S = MODE == OTH_PLAYOUT_MOVES ? (uint32_t)NN * (uint32_t)R : (uint32_t)R;
    const Eng eng(0, lds_rays);
    for (int base = chunk * BLOCK; base < limit; base += B * BLOCK) {  // block-uniform
        const int t = base + tid;
        const bool active = t < limit;
        const int q = active ? t / R : 0, r = active ? t - q * R : 0;
        int e = e0, a = 0, row = q;
        if constexpr (MODE == OTH_PLAYOUT_MOVES) {
            a = select_bit(root_moves, q);  // q < popcount for an active lane
            row = a;
        } else {
            e = e0 + q;
        }
        const uint32_t id = key.id_key + (key.id_base + (uint32_t)e) * S + (uint32_t)a * (uint32_t)R + (uint32_t)r;
        Lane<N> s;
        load_lane<N>(s, boards, meta, legal, e);
        s.meta &= M_TURN_WHITE | M_TERMINATED;  // opening plies left play no part
        const int root = (s.meta & M_TURN_WHITE) ? WHITE_DISK : BLACK_DISK;
        bool live = active && !(s.meta & M_TERMINATED);
        const bool counted = live;
        int outcome = NO_DISK;  // the winner's colour
        eng.prime(s);
        if constexpr (MODE == OTH_PLAYOUT_MOVES) {
            if (live) {  // the root move: oth_step with flags 0
                int rr, dd, win;
                step_lane<N, Eng, false>(s, a, 0u, rr, dd, win, eng);
                if (dd) {
                    live = false;
                    outcome = win;
                }
            }
        }
        // playout ply p draws word p % 4 of Philox block block0 + p / 4: four plies a block
        if constexpr (W == 1) {
            // one-word boards: the board as (mover, opponent) plus the side-to-move bit, as
            // k_play_rand holds it -- a ply swaps two words instead of selecting mover and
            // opponent from (black, white) and writing them back -- with step_lane's results:
            // a live board without a possible move (a stale or emptied possible_moves at
            // the root) takes the invalid path, flags 0: nothing is placed, the turn passes
            bool tw = (s.meta & M_TURN_WHITE) != 0;
            uint64_t M = tw ? s.white.w[0] : s.black.w[0], O = tw ? s.black.w[0] : s.white.w[0];
            uint64_t L = s.legal.w[0];  // (eng.t holds the fills of this mover: prime, or the root move's scan)
            auto fast = [&](uint32_t u) __attribute__((always_inline)) {
                if (live) {
                    const bool valid = L != 0;
                    const int pa = select64_tab(L, scale_index(u, popc64(L)), sel8);  // (< 64 for L == 0 too)
                    const uint64_t keep = 0ull - (uint64_t)valid;
                    BB<1> dummy;
                    dummy.w[0] = 0;
                    const uint64_t fl = eng.flip(dummy, dummy, pa).w[0] & keep;  // update_board
                    const uint64_t mv = (1ull << pa) & keep;
                    BB<1> pb, ob;
                    pb.w[0] = O & ~fl;       // the next mover
                    ob.w[0] = M | fl | mv;
                    uint64_t Ln = eng.legal(pb, ob).w[0];  // its possible_moves (none on a full board)
                    const bool pass = Ln == 0;
                    if (pass) Ln = eng.legal(ob, pb).w[0];  // the mover moves again (fills recomputed)
                    M = pass ? ob.w[0] : pb.w[0];
                    O = pass ? pb.w[0] : ob.w[0];
                    L = Ln;
                    tw ^= !pass;
                    live = Ln != 0;  // a full board, or nobody can move: the winner by count
                }
            };
            for (int p = 0; p < PLAYOUT_MAX_PLIES && __any(live); p += 4) {
                const U4 d4 = philox4(key.seed, id, key.block0 + (uint64_t)(p >> 2), RNG_ACTION);
                fast(d4.x);
                fast(d4.y);
                fast(d4.z);
                fast(d4.w);
            }
            s.white.w[0] = tw ? M : O;
            s.black.w[0] = tw ? O : M;
            outcome = sign_i32(popc64(s.white.w[0]) - popc64(s.black.w[0]));  // WHITE_DISK = +1 (flags 0: no sudden death)
        } else {
            auto ply = [&](uint32_t u) __attribute__((always_inline)) {
                if (live) {
                    int pa;
                    if constexpr (W <= 2) {
                        const int n = popcount(s.legal);
                        pa = n ? select_bit_tab(s.legal, scale_index(u, n), sel8) : -1;
                    } else {
                        pa = random_action<N>(s, u);
                    }
                    int rr, dd, win;
                    step_lane<N, Eng, true>(s, pa, 0u, rr, dd, win, eng);
                    if (dd) {
                        live = false;
                        outcome = win;
                    }
                }
            };
            for (int p = 0; p < PLAYOUT_MAX_PLIES && __any(live); p += 4) {
                const U4 d4 = philox4(key.seed, id, key.block0 + (uint64_t)(p >> 2), RNG_ACTION);
                ply(d4.x);
                ply(d4.y);
                ply(d4.z);
                ply(d4.w);
            }
        }
        // outcome and disc difference from the root mover's side
        const bool fin = counted && !live;
        const int res = fin ? outcome * root : 0;
        const int diff = fin ? (popcount(s.white) - popcount(s.black)) * root : 0;
        const unsigned long long fm = __ballot(fin);
        if (fm) {
            const int first = __ffsll(fm) - 1;
            const int row0 = __shfl(row, first, 64);
            if (__all(!fin || row == row0)) {  // one row for the whole wave: ballots and a wave sum, one lane adds
                const int nw = __popcll(__ballot(fin && res > 0)), nd = __popcll(__ballot(fin && res == 0));
                const int nl = __popcll(fm) - nw - nd;
                const int sc = (int)wave_sum((uint32_t)diff);
                if ((tid & 63) == first) {
                    if (nw) atomicAdd(&cnt[4 * row0 + 0], nw);
                    if (nd) atomicAdd(&cnt[4 * row0 + 1], nd);
                    if (nl) atomicAdd(&cnt[4 * row0 + 2], nl);
                    if (sc) atomicAdd(&cnt[4 * row0 + 3], sc);
                }
            } else if (fin) {  // several boards or squares in the wave (small R)
                atomicAdd(&cnt[4 * row + 1 - res], 1);
                if (diff) atomicAdd(&cnt[4 * row + 3], diff);
            }
        }
    }
    __syncthreads();
    // every element of the group's outputs once: a plain store, or an add into
    // the zeroed output where B blocks share the group
    const int rows = MODE == OTH_PLAYOUT_MOVES ? NN : ne;
    const size_t row_base = MODE == OTH_PLAYOUT_MOVES ? (size_t)e0 * NN : (size_t)e0;
    for (int i = tid; i < rows * 4; i += BLOCK) {
        const int j = i & 3, v = cnt[i];
        int32_t* dst = j < 3 ? wdl + (row_base + (size_t)(i >> 2)) * 3 + j : score + row_base + (size_t)(i >> 2);
        if (j == 3 && !score) continue;
        if (!split) *dst = v;
        else if (v) atomicAdd(dst, v);
    }
}

// The outputs of a call whose blocks add into them (B > 1).  A kernel, not hipMemsetAsync: captured
// into a HIP graph, the memset of a size that is no multiple of 8 bytes replayed with a wrong last word.
template <int N>
__global__ __launch_bounds__(BLOCK) void k_playout_zero(int32_t* __restrict__ wdl, size_t n_wdl,
                                                        int32_t* __restrict__ score, size_t n_score) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n_wdl) wdl[i] = 0;
    if (score && i < n_score) score[i] = 0;
}

// best[e] = the lowest legal square of the largest wins - losses; -1 for a
// terminated board or an empty possible_moves
template <int N>
__global__ __launch_bounds__(BLOCK) void k_playout_best(const uint16_t* __restrict__ meta,
                                                        const uint64_t* __restrict__ legal, int E,
                                                        const int32_t* __restrict__ wdl, int32_t* __restrict__ best) {
    constexpr int W = Geo<N>::W, NN = N * N;
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= E) return;
    int b = -1, bv = 0;
    if (!(meta[e] & M_TERMINATED)) {
        for (int w = 0; w < W; ++w) {
            uint64_t m = legal[(size_t)e * W + w];
            while (m) {
                const int a = 64 * w + __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                if (a >= NN) break;
                const int32_t* c = wdl + ((size_t)e * NN + a) * 3;
                const int v = c[0] - c[2];
                if (b < 0 || v > bv) {
                    b = a;
                    bv = v;
                }
            }
        }
    }
    best[e] = b;
}

}  // namespace oth_dev
