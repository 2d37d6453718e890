// solve.hpp -- oth_solve: exact endgame values and best moves (the spec is the
// header's comment on oth_solve).  G(pos, mover) is the final disc difference
// under best play by both sides, counted from the mover's side, with the
// reference's end-of-game rules (othello.py:424-442, 473-501).
//
// The search core (the part outside __HIPCC__) is plain host/device code over
// bitboard.hpp: tests/host/solve_host.cpp compiles the same text with g++.  It
// is a fail-soft alpha-beta negamax with an explicit stack, written as one
// *node step* (solve_step) that a driver repeats until the task is done:
//   * a finished node (no move left, or best >= beta) backs up one level;
//   * otherwise the node's next move (ascending squares) is placed and flipped,
//     and the child is a leaf by count (full board, nobody can move), a leaf by
//     the last-ply shortcut (one empty square: the flip count of that square
//     for the child's mover, or else for the other side; no board is updated,
//     no frame pushed), or is descended into;
//   * a pass is handled in place: the child's sides are swapped and its window
//     negated, with a flag in the frame that negates its value on the way up.
//     No frame is pushed for it, so the depth is at most the empty squares.
// A task is one root move: a pseudo-node whose only move is that square, with
// the full window, so its value is exact whatever the other root moves give.
// A node is a position reached by placing a disc; the budget (max_nodes) is per
// task and is checked before every placement.
//
// Device mapping (k_solve): one lane per (board, root move) task.  A block is
// one wave and serves SOLVE_GROUP consecutive boards: it builds the prefix of
// their task counts (popcount of the stored possible_moves: device data) in
// LDS, packs the tasks densely over its lanes, and loops over 64-task chunks
// until the group's tasks are done; inside a chunk the lanes repeat the node
// step while any of them is live.  A board's tasks never leave its block, so
// value / best / status / nodes are reduced in LDS (an integer max and sums:
// the order of arrival does not show) and no second kernel is needed.
//
// Stack.  A per-lane array of max 14 frames (scratch
// memory, as maximin_value's), FRAME = 6 W + 1 dwords: mover, opponent, remaining
// moves, and alpha / beta / best / pass packed.  The other arm, one-word boards'
// stack in LDS laid out [(level * FRAME + k) * 64 + lane] (64 distinct banks a
// wave access whatever level each lane is at), is kept behind
// OTH_SOLVE_LDS_STACK: it measured slower.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "bitboard.hpp"

namespace oth {

constexpr int SOLVE_MAX_EMPTIES = 14;   // OTH_SOLVE_MAX_EMPTIES
constexpr int SOLVE_NO_VALUE = -32768;  // OTH_SOLVE_NO_VALUE
constexpr int SOLVE_EXACT = 0, SOLVE_TERMINATED = 1, SOLVE_SKIPPED = 2, SOLVE_NO_MOVE = 3, SOLVE_ABORTED = 4;

// update_board's flips (othello.py:391-410) of a move on square a of a one-word
// board from the two sides' discs alone (no fills: the search comes back to a
// node whose scan is long gone).  Per direction toward higher squares the ray
// is ray0(S) << a without edge masks, the run the ray's squares before its
// first square outside Oin (y's lowest bit; y - 1 every bit below it), kept if
// that square holds an own disc.  Off the vertical axis Oin = O & INNER: a ray
// can leave its row only through an edge-column square, which Oin does not
// hold, so y's lowest bit lies at or before the wrap (a ray starting on the
// edge column wraps at once and its run is empty).  The vertical ray runs off
// the board onto squares that hold no disc.  Toward lower squares the same on
// the board turned by 180 degrees.  a in [0, N*N).
template <int N>
OTH_HD uint64_t solve_flips1(uint64_t P, uint64_t O, int a) {
    using OW = OneWord<N>;
    constexpr uint64_t RAY[4] = {OW::RAY_E, OW::RAY_S, OW::RAY_SE, OW::RAY_SW};
    const uint32_t su = (uint32_t)a & 63u, sd = (uint32_t)(N * N - 1 - a) & 63u;
    const uint64_t Pt = OW::turn180(P), Ot = OW::turn180(O);
    uint64_t f = 0, g = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint64_t in = d == 1 ? OW::BD : OW::IN;
        const uint64_t ou = O & in, od = Ot & in;
        const uint64_t ru = RAY[d] << su, rd = RAY[d] << sd;
        const uint64_t yu = ru & ~ou, yd = rd & ~od;
        const uint64_t capu = andn_and_64(yu, yu - 1ull, P), capd = andn_and_64(yd, yd - 1ull, Pt);
        f |= capu ? and3_64(ru, ou, yu - 1ull) : 0ull;
        g |= capd ? and3_64(rd, od, yd - 1ull) : 0ull;
    }
    return f | OW::turn180(g);
}

template <int N>
OTH_HD BB<Geo<N>::W> solve_flips(const BB<Geo<N>::W>& P, const BB<Geo<N>::W>& O, int a) {
    if constexpr (Geo<N>::W == 1) {
        BB<1> r;
        r.w[0] = solve_flips1<N>(P.w[0], O.w[0], a);
        return r;
    } else {
        return flips<N>(P, O, square<Geo<N>::W>(a));
    }
}

template <int N>
OTH_HD BB<Geo<N>::W> solve_legal(const BB<Geo<N>::W>& P, const BB<Geo<N>::W>& O) {
    if constexpr (Geo<N>::W == 1) {
        uint64_t t[8];  // the fills are dead here
        BB<1> r;
        r.w[0] = OneWord<N>::legal(P.w[0], O.w[0], t);
        return r;
    } else {
        return legal_moves<N>(P, O);
    }
}

// the lowest square of a non-empty board
template <int W>
OTH_HD int lowest_square(const BB<W>& b) {
    int res = 0;
#pragma unroll
    for (int i = W - 1; i >= 0; --i)
        if (b.w[i]) res = 64 * i + ctz64(b.w[i]);
    return res;
}

// What a board gets without a search: its status and, for a terminated board,
// its value.  black / white / stored: the handle's words; meta: its meta word.
template <int N>
OTH_HD int solve_status(const BB<Geo<N>::W>& black, const BB<Geo<N>::W>& white, const BB<Geo<N>::W>& stored,
                        uint32_t meta, int max_empties, int& value) {
    const int nb = popcount(black), nw = popcount(white);
    value = SOLVE_NO_VALUE;
    if (meta & 2u) {  // terminated: the discs of the side in the turn bit minus the other's
        value = (meta & 1u) ? nw - nb : nb - nw;
        return SOLVE_TERMINATED;
    }
    if (N * N - popcount(black | white) > max_empties) return SOLVE_SKIPPED;
    if (!any(stored & Geo<N>::BOARD)) return SOLVE_NO_MOVE;
    return SOLVE_EXACT;
}

// A frame: the node's mover, opponent and remaining moves as dwords, then
// alpha / beta / best (each + 512, 10 bits) and the pass flag in one dword.
template <int N>
struct SolveFrame {
    static constexpr int W = Geo<N>::W;
    static constexpr int DWORDS = 6 * W + 1;
    static constexpr int INF = N * N + 1;
};

// A per-lane stack as a plain array (the host build, and multi-word boards on
// the device, where its dynamic index puts it into scratch memory).
template <int WORDS>
struct SolveArrayStack {
    uint32_t s[WORDS];
    OTH_HD uint32_t get(int i) const { return s[i]; }
    OTH_HD void put(int i, uint32_t v) { s[i] = v; }
};

template <int N>
struct SolveTask {
    static constexpr int W = Geo<N>::W;
    BB<W> M, O, R;  // the current node: mover, opponent, moves not yet taken
    int alpha, beta, best;
    bool pass;  // the node's sides were swapped by a pass: its value is negated on the way up
    int sp;     // frames on the stack
    uint32_t nodes;
    bool over;  // the budget ran out: the task is abandoned
    bool live;
    int result;  // -G(after the root move, other side), once !live && !over
};

// the task of root move a: a pseudo-node with that one move and the full window
template <int N>
OTH_HD void solve_task_init(SolveTask<N>& s, const BB<Geo<N>::W>& mover, const BB<Geo<N>::W>& opp, int a) {
    s.M = mover;
    s.O = opp;
    s.R = square<Geo<N>::W>(a);
    s.alpha = -SolveFrame<N>::INF;
    s.beta = SolveFrame<N>::INF;
    s.best = -SolveFrame<N>::INF;
    s.pass = false;
    s.sp = 0;
    s.nodes = 0;
    s.over = false;
    s.live = true;
    s.result = 0;
}

template <int N, typename Stack>
OTH_HD void solve_push(const SolveTask<N>& s, Stack& st) {
    constexpr int W = Geo<N>::W, F = SolveFrame<N>::DWORDS;
    const int at = s.sp * F;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        st.put(at + 6 * i + 0, (uint32_t)s.M.w[i]);
        st.put(at + 6 * i + 1, (uint32_t)(s.M.w[i] >> 32));
        st.put(at + 6 * i + 2, (uint32_t)s.O.w[i]);
        st.put(at + 6 * i + 3, (uint32_t)(s.O.w[i] >> 32));
        st.put(at + 6 * i + 4, (uint32_t)s.R.w[i]);
        st.put(at + 6 * i + 5, (uint32_t)(s.R.w[i] >> 32));
    }
    st.put(at + 6 * W, (uint32_t)(s.alpha + 512) | (uint32_t)(s.beta + 512) << 10 | (uint32_t)(s.best + 512) << 20 |
                           (uint32_t)s.pass << 30);
}

template <int N, typename Stack>
OTH_HD void solve_pop(SolveTask<N>& s, const Stack& st) {
    constexpr int W = Geo<N>::W, F = SolveFrame<N>::DWORDS;
    const int at = s.sp * F;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        s.M.w[i] = (uint64_t)st.get(at + 6 * i + 1) << 32 | st.get(at + 6 * i + 0);
        s.O.w[i] = (uint64_t)st.get(at + 6 * i + 3) << 32 | st.get(at + 6 * i + 2);
        s.R.w[i] = (uint64_t)st.get(at + 6 * i + 5) << 32 | st.get(at + 6 * i + 4);
    }
    const uint32_t p = st.get(at + 6 * W);
    s.alpha = (int)(p & 1023u) - 512;
    s.beta = (int)((p >> 10) & 1023u) - 512;
    s.best = (int)((p >> 20) & 1023u) - 512;
    s.pass = ((p >> 30) & 1u) != 0;
}

// One placement against the budget: false (and the task abandoned) when the
// task has already placed max_nodes discs.
template <int N>
OTH_HD bool solve_count(SolveTask<N>& s, uint32_t max_nodes) {
    if (s.nodes == max_nodes) {
        s.over = true;
        s.live = false;
        return false;
    }
    ++s.nodes;
    return true;
}

// One node step of a live task (see the top of the file).  levels: the frames
// the stack holds; a search never needs more than the root's empty squares.
template <int N, typename Stack>
OTH_HD void solve_step(SolveTask<N>& s, Stack& st, uint32_t max_nodes, int levels) {
    constexpr int W = Geo<N>::W, NN = N * N, INF = SolveFrame<N>::INF;
    if (!any(s.R) || s.best >= s.beta) {  // the node is finished: back up one level
        const int v = s.pass ? -s.best : s.best;
        if (s.sp == 0) {
            s.result = v;
            s.live = false;
            return;
        }
        --s.sp;
        solve_pop<N>(s, st);
        s.best = s.best > -v ? s.best : -v;
        if (!any(s.R) || s.best >= s.beta) return;  // the parent is finished too: the next step's
    }
    if (!solve_count<N>(s, max_nodes)) return;
    const int a = lowest_square<W>(s.R);
    const BB<W> bit = square<W>(a);
    s.R = s.R & ~bit;
    const BB<W> fl = solve_flips<N>(s.M, s.O, a);
    const BB<W> Mn = s.M | fl | bit, On = s.O & ~fl;  // the child: On to move against Mn
    const int cm = popcount(Mn), co = popcount(On);
    const int empties = NN - popcount(Mn | On);
    int v = cm - co;  // a leaf by count, from this node's mover's side
    bool leaf = true;
    if (empties == 1) {  // the last ply: the flip count of the one square, no board updated
        const int sq = lowest_square<W>(~(Mn | On) & Geo<N>::BOARD);
        const int n1 = popcount(solve_flips<N>(On, Mn, sq));
        if (n1) {
            if (!solve_count<N>(s, max_nodes)) return;
            v = cm - co - 1 - 2 * n1;
        } else {
            const int n2 = popcount(solve_flips<N>(Mn, On, sq));
            if (n2) {
                if (!solve_count<N>(s, max_nodes)) return;
                v = cm - co + 1 + 2 * n2;
            }
        }
    } else if (empties > 1) {
        BB<W> Lc = solve_legal<N>(On, Mn);
        bool passed = false;
        if (!any(Lc)) {  // the child's mover has no move: the other side moves again, or the game is over
            Lc = solve_legal<N>(Mn, On);
            passed = true;
        }
        if (any(Lc)) {
            if (s.sp >= levels) {  // (never: levels covers the empty squares; kept for memory safety)
                s.over = true;
                s.live = false;
                return;
            }
            leaf = false;
            solve_push<N>(s, st);
            ++s.sp;
            const int lo = s.alpha > s.best ? s.alpha : s.best;
            s.alpha = passed ? lo : -s.beta;  // the child's window is (-beta, -lo); a pass negates it again
            s.beta = passed ? s.beta : -lo;
            s.best = -INF;
            s.pass = passed;
            s.M = passed ? Mn : On;
            s.O = passed ? On : Mn;
            s.R = Lc;
        }
    }
    if (leaf) s.best = s.best > v ? s.best : v;
}

// One board on the host (the tests' host build and the probe's single-thread
// figure): the spec's outputs for one board, the tasks in ascending squares.
// move_values: N*N entries.  Returns the status.
template <int N>
inline int solve_board_host(const uint64_t* black, const uint64_t* white, const uint64_t* stored, uint32_t meta,
                            int max_empties, uint32_t max_nodes, int32_t* value, int32_t* best,
                            int32_t* move_values, uint64_t* nodes) {
    constexpr int W = Geo<N>::W, NN = N * N;
    BB<W> B, Wt, Lg;
    for (int i = 0; i < W; ++i) {
        B.w[i] = black[i];
        Wt.w[i] = white[i];
        Lg.w[i] = stored[i];
    }
    for (int a = 0; a < NN; ++a) move_values[a] = SOLVE_NO_VALUE;
    *best = -1;
    *nodes = 0;
    int v0;
    const int status = solve_status<N>(B, Wt, Lg, meta, max_empties, v0);
    *value = v0;
    if (status != SOLVE_EXACT) return status;
    const bool tw = (meta & 1u) != 0;
    const BB<W> mover = tw ? Wt : B, opp = tw ? B : Wt;
    BB<W> todo = Lg & Geo<N>::BOARD;
    bool aborted = false;
    int bv = -SolveFrame<N>::INF, ba = -1;
    static thread_local SolveArrayStack<SOLVE_MAX_EMPTIES * SolveFrame<N>::DWORDS> st;
    while (any(todo)) {
        const int a = lowest_square<W>(todo);
        todo = todo & ~square<W>(a);
        SolveTask<N> s;
        solve_task_init<N>(s, mover, opp, a);
        while (s.live) solve_step<N>(s, st, max_nodes, max_empties);
        *nodes += (uint64_t)s.nodes + (s.over ? 1u : 0u);
        if (s.over) {
            aborted = true;
            continue;
        }
        move_values[a] = s.result;
        if (s.result > bv) {
            bv = s.result;
            ba = a;
        }
    }
    if (aborted) return SOLVE_ABORTED;
    *value = bv;
    *best = ba;
    return SOLVE_EXACT;
}

}  // namespace oth

#if defined(__HIPCC__)
#include "state.hpp"

namespace oth_dev {

// 0: every board size keeps the stack in a per-lane array (scratch memory); 1 (the
// other arm of DESIGN.md section 4's comparison, slower at 65,536 boards):
// one-word boards keep it in LDS, SolveLdsStack
#ifndef OTH_SOLVE_LDS_STACK
#define OTH_SOLVE_LDS_STACK 0
#endif

constexpr int SOLVE_BLOCK = 64;  // one wave a block
constexpr int SOLVE_GROUP = 8;   // boards a block: about a wave of tasks late in the game

static_assert(SOLVE_MAX_EMPTIES == OTH_SOLVE_MAX_EMPTIES && SOLVE_NO_VALUE == OTH_SOLVE_NO_VALUE, "the header's");
static_assert(SOLVE_EXACT == OTH_SOLVE_EXACT && SOLVE_TERMINATED == OTH_SOLVE_TERMINATED &&
                  SOLVE_SKIPPED == OTH_SOLVE_SKIPPED && SOLVE_NO_MOVE == OTH_SOLVE_NO_MOVE &&
                  SOLVE_ABORTED == OTH_SOLVE_ABORTED,
              "the header's status codes");

// the per-lane stack in LDS: dword i of lane l at [i * 64 + l]
struct SolveLdsStack {
    uint32_t* p;  // the lane's column
    __device__ __forceinline__ uint32_t get(int i) const { return p[i * SOLVE_BLOCK]; }
    __device__ __forceinline__ void put(int i, uint32_t v) { p[i * SOLVE_BLOCK] = v; }
};

// dynamic LDS of a launch: the one-word boards' stacks
template <int N>
constexpr size_t solve_lds_bytes(int levels) {
    return Geo<N>::W == 1 && OTH_SOLVE_LDS_STACK ? (size_t)levels * SolveFrame<N>::DWORDS * SOLVE_BLOCK * sizeof(uint32_t) : 0;
}

template <int N>
__global__ __launch_bounds__(SOLVE_BLOCK) void k_solve(const uint64_t* __restrict__ boards,
                                                       const uint16_t* __restrict__ meta,
                                                       const uint64_t* __restrict__ legal, int E, int max_empties,
                                                       uint32_t max_nodes, int32_t* __restrict__ value,
                                                       int32_t* __restrict__ best, int32_t* __restrict__ move_values,
                                                       uint8_t* __restrict__ status,
                                                       unsigned long long* __restrict__ nodes) {
    constexpr int W = Geo<N>::W, NN = N * N, G = SOLVE_GROUP;
    static_assert(NN <= 256, "a square fits the reduction key's low byte");
    extern __shared__ uint32_t lds_stack[];
    __shared__ uint64_t g_moves[G][W];  // the searched boards' stored possible_moves; none for the others
    __shared__ int g_cnt[G];
    __shared__ int g_key[G];            // max of (value + 512) << 8 | (255 - square): the lowest square of the best value
    __shared__ unsigned int g_over[G];
    __shared__ unsigned long long g_nodes[G];
    __shared__ int g_status[G];
    const int lane = threadIdx.x;
    const long long e0 = (long long)blockIdx.x * G;
    const int ne = (int)(E - e0 < G ? E - e0 : G);
    if (lane < G) {
        BB<W> mv = zero<W>();
        int st = SOLVE_SKIPPED;
        if (lane < ne) {
            const size_t e = (size_t)(e0 + lane);
            BB<W> B, Wt, Lg;
#pragma unroll
            for (int i = 0; i < W; ++i) {
                B.w[i] = boards[e * 2 * W + i];
                Wt.w[i] = boards[e * 2 * W + W + i];
                Lg.w[i] = legal[e * W + i];
            }
            int v;
            st = solve_status<N>(B, Wt, Lg, meta[e], max_empties, v);
            if (st == SOLVE_EXACT) {
                mv = Lg & Geo<N>::BOARD;
            } else {  // no search: every output of the board here
                value[e] = v;
                if (best) best[e] = -1;
                if (status) status[e] = (uint8_t)st;
                if (nodes) nodes[e] = 0ull;
            }
        }
#pragma unroll
        for (int i = 0; i < W; ++i) g_moves[lane][i] = mv.w[i];
        g_cnt[lane] = popcount(mv);
        g_key[lane] = -1;
        g_over[lane] = 0u;
        g_nodes[lane] = 0ull;
        g_status[lane] = st;
    }
    __syncthreads();
    int pre[G + 1];  // the prefix of the group's task counts
    pre[0] = 0;
#pragma unroll
    for (int i = 0; i < G; ++i) pre[i + 1] = pre[i] + g_cnt[i];
    const int total = pre[G];
    if (move_values)  // NO_VALUE on every square that is no task; the tasks store their own
        for (int j = lane; j < ne * NN; j += SOLVE_BLOCK) {
            const int i = j / NN, a = j - i * NN;
            BB<W> mv;
#pragma unroll
            for (int k = 0; k < W; ++k) mv.w[k] = g_moves[i][k];
            if (!test(mv, a)) move_values[(size_t)(e0 + i) * NN + a] = SOLVE_NO_VALUE;
        }
    for (int base = 0; base < total; base += SOLVE_BLOCK) {  // block-uniform
        const int t = base + lane;
        const bool active = t < total;
        int i = 0;  // the task's board: the last i with pre[i] <= t
#pragma unroll
        for (int k = 1; k < G; ++k) i += (active && t >= pre[k]) ? 1 : 0;
        int first = 0;
#pragma unroll
        for (int k = 1; k < G; ++k) first = i >= k ? pre[k] : first;
        const size_t e = (size_t)(e0 + i);  // (i < ne: boards past E have no task)
        BB<W> B, Wt, mv;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            B.w[k] = boards[e * 2 * W + k];
            Wt.w[k] = boards[e * 2 * W + W + k];
            mv.w[k] = g_moves[i][k];
        }
        const bool tw = (meta[e] & M_TURN_WHITE) != 0;
        const int a = active ? select_bit(mv, t - first) : 0;  // (t - first < popcount for an active lane)
        SolveTask<N> s;
        solve_task_init<N>(s, pick(tw, Wt, B), pick(tw, B, Wt), a);
        s.live = active;
        if constexpr (W == 1 && OTH_SOLVE_LDS_STACK) {
            SolveLdsStack st{lds_stack + lane};
            while (__any(s.live))
                if (s.live) solve_step<N>(s, st, max_nodes, max_empties);
        } else {
            SolveArrayStack<SOLVE_MAX_EMPTIES * SolveFrame<N>::DWORDS> st;
            while (__any(s.live))
                if (s.live) solve_step<N>(s, st, max_nodes, max_empties);
        }
        if (active) {
            if (s.over) atomicOr(&g_over[i], 1u);
            else atomicMax(&g_key[i], ((s.result + 512) << 8) | (255 - a));
            atomicAdd(&g_nodes[i], (unsigned long long)s.nodes + (s.over ? 1ull : 0ull));
            if (move_values) move_values[e * NN + a] = s.over ? SOLVE_NO_VALUE : s.result;
        }
    }
    __syncthreads();
    if (lane < ne && g_status[lane] == SOLVE_EXACT) {
        const size_t e = (size_t)(e0 + lane);
        const bool over = g_over[lane] != 0u;
        const int key = g_key[lane];
        value[e] = over ? SOLVE_NO_VALUE : (key >> 8) - 512;
        if (best) best[e] = over ? -1 : 255 - (key & 255);
        if (status) status[e] = (uint8_t)(over ? SOLVE_ABORTED : SOLVE_EXACT);
        if (nodes) nodes[e] = g_nodes[lane];
    }
}

}  // namespace oth_dev
#endif
