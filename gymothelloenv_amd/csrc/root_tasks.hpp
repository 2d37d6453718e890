// root_tasks.hpp -- the layer under oth_solve, oth_search and the search
// players (solve.hpp, search.hpp, play_search.hpp; a header of its own, since
// all three stand on it): a fail-soft alpha-beta negamax over one *task* per
// root move, written as one *node step* that a driver repeats until the task
// is done.
//   * a finished node (no move left, or best >= beta) backs up one level
//     (node_backup);
//   * otherwise the node's next move (ascending squares) is placed and flipped
//     against the budget (node_place), and the search's own leaf rule decides
//     whether the child is a leaf or is descended into (node_descend);
//   * a pass is handled in place: the child's sides are swapped and its window
//     negated, with a flag in the frame that negates its value on the way up.
//     No frame is pushed for it.
// A task is one root move: a pseudo-node whose only move is that square, with
// the full window, so its value is exact whatever the other root moves give.
// A node is a position reached by placing a disc; the budget (max_nodes) is per
// task and is checked before every placement.
//
// A search supplies a Frame (its constants DWORDS, STACK_DWORDS, INF and
// NO_VALUE, and its packing of alpha / beta / best / pass behind the 6 W board
// dwords) and a step built from the three blocks with its leaf rule between
// them.  The part outside __HIPCC__ is plain host/device code over
// bitboard.hpp: tests/host/*.cpp compile the same text with g++,
// root_moves_host being one board's driver there.
//
// Device mapping (run_tasks, root_tasks_kernel): one lane per (board, root
// move) task.  A block is one wave and serves SOLVE_GROUP consecutive boards:
// it builds the prefix of their task counts in LDS, packs the tasks densely
// over its lanes, and loops over 64-task chunks until the group's tasks are
// done; inside a chunk the lanes repeat the node step while any of them is
// live.  A board's tasks never leave its block, so value / best / status /
// nodes are reduced in LDS (an integer max and sums: the order of arrival does
// not show) and no second kernel is needed.  The stack is a per-lane array of
// frames (scratch memory, as maximin_value's).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "bitboard.hpp"

namespace oth {

// the statuses every search shares: searched to the end, and over its budget
constexpr int ROOT_SEARCHED = 0, ROOT_ABORTED = 4;

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

template <int N>
struct RootTask {
    static constexpr int W = Geo<N>::W;
    BB<W> M, O, R;  // the current node: mover, opponent, moves not yet taken
    int alpha, beta, best;
    bool pass;  // the node's sides were swapped by a pass: its value is negated on the way up
    int sp;     // frames on the stack
    uint32_t nodes;
    bool over;  // the budget ran out: the task is abandoned
    bool live;
    int result;  // -(the value after the root move, other side), once !live && !over
};

// the task of root move a: a pseudo-node with that one move and the full window (-inf, inf)
template <int N>
OTH_HD void task_init(RootTask<N>& s, const BB<Geo<N>::W>& mover, const BB<Geo<N>::W>& opp, int a, int inf) {
    s.M = mover;
    s.O = opp;
    s.R = square<Geo<N>::W>(a);
    s.alpha = -inf;
    s.beta = inf;
    s.best = -inf;
    s.pass = false;
    s.sp = 0;
    s.nodes = 0;
    s.over = false;
    s.live = true;
    s.result = 0;
}

// A frame: the node's mover, opponent and remaining moves as 6 W dwords, then
// the search's own packing of alpha / beta / best / pass (Frame::pack / unpack).
// st: the task's stack, a plain array of frames sized by its user.
template <int N, typename Frame>
OTH_HD void frame_push(const RootTask<N>& s, uint32_t* st) {
    constexpr int W = Geo<N>::W;
    uint32_t* f = st + s.sp * Frame::DWORDS;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        f[6 * i + 0] = (uint32_t)s.M.w[i];
        f[6 * i + 1] = (uint32_t)(s.M.w[i] >> 32);
        f[6 * i + 2] = (uint32_t)s.O.w[i];
        f[6 * i + 3] = (uint32_t)(s.O.w[i] >> 32);
        f[6 * i + 4] = (uint32_t)s.R.w[i];
        f[6 * i + 5] = (uint32_t)(s.R.w[i] >> 32);
    }
    Frame::pack(s, f + 6 * W);
}

template <int N, typename Frame>
OTH_HD void frame_pop(RootTask<N>& s, const uint32_t* st) {
    constexpr int W = Geo<N>::W;
    const uint32_t* f = st + s.sp * Frame::DWORDS;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        s.M.w[i] = (uint64_t)f[6 * i + 1] << 32 | f[6 * i + 0];
        s.O.w[i] = (uint64_t)f[6 * i + 3] << 32 | f[6 * i + 2];
        s.R.w[i] = (uint64_t)f[6 * i + 5] << 32 | f[6 * i + 4];
    }
    Frame::unpack(s, f + 6 * W);
}

// One placement against the budget: false (and the task abandoned) when the
// task has already placed max_nodes discs.
template <int N>
OTH_HD bool task_count(RootTask<N>& s, uint32_t max_nodes) {
    if (s.nodes == max_nodes) {
        s.over = true;
        s.live = false;
        return false;
    }
    ++s.nodes;
    return true;
}

// the task is abandoned (the steps' stack guards)
template <int N>
OTH_HD void task_abandon(RootTask<N>& s) {
    s.over = true;
    s.live = false;
}

// The first block of a node step: a finished node backs up one level, its
// value folded into the parent.  True: the step is over (the task is done, or
// the parent is finished too, which is the next step's).
template <int N, typename Frame>
OTH_HD bool node_backup(RootTask<N>& s, const uint32_t* st) {
    if (any(s.R) && s.best < s.beta) return false;
    const int v = s.pass ? -s.best : s.best;
    if (s.sp == 0) {
        s.result = v;
        s.live = false;
        return true;
    }
    --s.sp;
    frame_pop<N, Frame>(s, st);
    s.best = s.best > -v ? s.best : -v;
    return !any(s.R) || s.best >= s.beta;
}

// The second: the node's lowest remaining move is counted against the budget,
// placed and flipped.  The child is On to move against Mn.  False: over budget.
template <int N>
OTH_HD bool node_place(RootTask<N>& s, uint32_t max_nodes, BB<Geo<N>::W>& Mn, BB<Geo<N>::W>& On) {
    constexpr int W = Geo<N>::W;
    if (!task_count<N>(s, max_nodes)) return false;
    const int a = lowest_square<W>(s.R);
    const BB<W> bit = square<W>(a);
    s.R = s.R & ~bit;
    const BB<W> fl = solve_flips<N>(s.M, s.O, a);
    Mn = s.M | fl | bit;
    On = s.O & ~fl;
    return true;
}

// The last: the task goes down into the child (the caller has seen to the
// frame's room).  moves: those of the side that moves there; passed: that side
// is Mn, the child's mover having none.
template <int N, typename Frame>
OTH_HD void node_descend(RootTask<N>& s, uint32_t* st, const BB<Geo<N>::W>& Mn, const BB<Geo<N>::W>& On,
                         const BB<Geo<N>::W>& moves, bool passed) {
    frame_push<N, Frame>(s, st);
    ++s.sp;
    const int lo = s.alpha > s.best ? s.alpha : s.best;
    s.alpha = passed ? lo : -s.beta;  // the child's window is (-beta, -lo); a pass negates it again
    s.beta = passed ? s.beta : -lo;
    s.best = -Frame::INF;
    s.pass = passed;
    s.M = passed ? Mn : On;
    s.O = passed ? On : Mn;
    s.R = moves;
}

// One board on the host (the tests' host builds and the probes' single-thread
// figures): the spec's outputs for one board, its root moves in ascending
// squares, the best the first maximum.  status(B, W, stored, meta, v): what the
// board gets without a search; step(task, stack): the search's node step;
// move_values: N*N entries.  Returns the status.
template <int N, typename Frame, typename Status, typename Step>
inline int root_moves_host(const uint64_t* black, const uint64_t* white, const uint64_t* stored, uint32_t meta,
                           Status status, Step step, int32_t* value, int32_t* best, int32_t* move_values,
                           uint64_t* nodes) {
    constexpr int W = Geo<N>::W, NN = N * N;
    BB<W> B, Wt, Lg;
    for (int i = 0; i < W; ++i) {
        B.w[i] = black[i];
        Wt.w[i] = white[i];
        Lg.w[i] = stored[i];
    }
    for (int a = 0; a < NN; ++a) move_values[a] = Frame::NO_VALUE;
    *best = -1;
    *nodes = 0;
    int v0;
    const int st0 = status(B, Wt, Lg, meta, v0);
    *value = v0;
    if (st0 != ROOT_SEARCHED) return st0;
    const bool tw = (meta & 1u) != 0;
    const BB<W> mover = tw ? Wt : B, opp = tw ? B : Wt;
    BB<W> todo = Lg & Geo<N>::BOARD;
    bool aborted = false;
    int bv = -Frame::INF, ba = -1;
    static thread_local uint32_t st[Frame::STACK_DWORDS];
    while (any(todo)) {
        const int a = lowest_square<W>(todo);
        todo = todo & ~square<W>(a);
        RootTask<N> s;
        task_init<N>(s, mover, opp, a, Frame::INF);
        while (s.live) step(s, st);
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
    if (aborted) return ROOT_ABORTED;
    *value = bv;
    *best = ba;
    return ROOT_SEARCHED;
}

}  // namespace oth

#if defined(__HIPCC__)
#include "state.hpp"

namespace oth_dev {

constexpr int SOLVE_BLOCK = 64;  // one wave a block
constexpr int SOLVE_GROUP = 8;   // boards a block: about a wave of tasks late in the game

// The key of a board's best root move: the max of (value + inf) << 8 |
// (255 - square) is the lowest square of the best value.  0: no task yet.
__device__ __forceinline__ unsigned long long root_key(int value, int inf, int a) {
    return (unsigned long long)(value + inf) << 8 | (unsigned long long)(255 - a);
}
__device__ __forceinline__ int root_key_value(unsigned long long key, int inf) { return (int)(key >> 8) - inf; }
__device__ __forceinline__ int root_key_square(unsigned long long key) { return 255 - (int)(key & 255ull); }

// The tasks of a group, SOLVE_BLOCK at a time.  g_moves, g_cnt: the SOLVE_GROUP
// boards' root moves and their counts in LDS, written before a barrier.
// load(i, a, active, M, O) gives the mover and opponent of board i, whose root
// move a is the lane's task if active, and returns the node step of its tasks,
// a callable (task, stack); done(task, i, a) takes the finished or abandoned
// task.  Returns the group's task count (block-uniform, as the chunk loop is).
template <int N, typename Frame, typename Load, typename Done>
__device__ __forceinline__ int run_tasks(const uint64_t (*g_moves)[Geo<N>::W], const int* g_cnt, Load load,
                                         Done done) {
    constexpr int W = Geo<N>::W, G = SOLVE_GROUP;
    const int lane = threadIdx.x;
    int pre[G + 1];  // the prefix of the group's task counts
    pre[0] = 0;
#pragma unroll
    for (int i = 0; i < G; ++i) pre[i + 1] = pre[i] + g_cnt[i];
    const int total = pre[G];
    for (int base = 0; base < total; base += SOLVE_BLOCK) {
        const int t = base + lane;
        const bool active = t < total;
        int i = 0;  // the task's board: the last i with pre[i] <= t
#pragma unroll
        for (int k = 1; k < G; ++k) i += (active && t >= pre[k]) ? 1 : 0;
        int first = 0;
#pragma unroll
        for (int k = 1; k < G; ++k) first = i >= k ? pre[k] : first;
        BB<W> M, O, mv;
#pragma unroll
        for (int k = 0; k < W; ++k) mv.w[k] = g_moves[i][k];
        const int a = active ? select_bit(mv, t - first) : 0;  // (t - first < popcount for an active lane)
        const auto step = load(i, a, active, M, O);
        RootTask<N> s;
        task_init<N>(s, M, O, a, Frame::INF);
        s.live = active;
        alignas(4) uint32_t st[Frame::STACK_DWORDS];  // (as declared: no rounding of the scratch to 16 bytes)
        while (__any(s.live))
            if (s.live) step(s, st);
        if (active) done(s, i, a);
    }
    return total;
}

// The body of k_solve and k_search: the group's boards classified by the lanes
// < SOLVE_GROUP, their tasks searched, the outputs stored by those lanes.
// status(B, W, stored, meta, v): what a board gets without a search;
// step(task, stack): the node step.  LDS the caller wrote before the call (the
// evaluation's planes) is readable in step: the barrier after the
// classification covers it.
template <int N, typename Frame, typename Status, typename Step>
__device__ __forceinline__ void root_tasks_kernel(const uint64_t* __restrict__ boards,
                                                  const uint16_t* __restrict__ meta,
                                                  const uint64_t* __restrict__ legal, int E,
                                                  int32_t* __restrict__ value, int32_t* __restrict__ best,
                                                  int32_t* __restrict__ move_values, uint8_t* __restrict__ status,
                                                  unsigned long long* __restrict__ nodes, Status status_of, Step step) {
    constexpr int W = Geo<N>::W, NN = N * N, G = SOLVE_GROUP;
    static_assert(NN <= 256, "a square fits the reduction key's low byte");
    __shared__ uint64_t g_moves[G][W];  // the searched boards' stored possible_moves; none for the others
    __shared__ int g_cnt[G];
    __shared__ unsigned long long g_key[G];
    __shared__ unsigned int g_over[G];
    __shared__ unsigned long long g_nodes[G];
    __shared__ int g_status[G];
    const int lane = threadIdx.x;
    const long long e0 = (long long)blockIdx.x * G;
    const int ne = (int)(E - e0 < G ? E - e0 : G);
    if (lane < G) {
        BB<W> mv = zero<W>();
        int st = ROOT_ABORTED;  // (a board past E: anything but ROOT_SEARCHED)
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
            st = status_of(B, Wt, Lg, meta[e], v);
            if (st == ROOT_SEARCHED) {
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
        g_key[lane] = 0ull;
        g_over[lane] = 0u;
        g_nodes[lane] = 0ull;
        g_status[lane] = st;
    }
    __syncthreads();
    if (move_values)  // NO_VALUE on every square that is no task; the tasks store their own
        for (int j = lane; j < ne * NN; j += SOLVE_BLOCK) {
            const int i = j / NN, a = j - i * NN;
            BB<W> mv;
#pragma unroll
            for (int k = 0; k < W; ++k) mv.w[k] = g_moves[i][k];
            if (!test(mv, a)) move_values[(size_t)(e0 + i) * NN + a] = Frame::NO_VALUE;
        }
    run_tasks<N, Frame>(
        g_moves, g_cnt,
        [&](int i, int, bool, BB<W>& M, BB<W>& O) {
            const size_t e = (size_t)(e0 + i);  // (i < ne: boards past E have no task)
            BB<W> B, Wt;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                B.w[k] = boards[e * 2 * W + k];
                Wt.w[k] = boards[e * 2 * W + W + k];
            }
            const bool tw = (meta[e] & M_TURN_WHITE) != 0;
            M = pick(tw, Wt, B);
            O = pick(tw, B, Wt);
            return step;
        },
        [&](const RootTask<N>& s, int i, int a) {
            if (s.over) atomicOr(&g_over[i], 1u);
            else atomicMax(&g_key[i], root_key(s.result, Frame::INF, a));
            atomicAdd(&g_nodes[i], (unsigned long long)s.nodes + (s.over ? 1ull : 0ull));
            if (move_values) move_values[(size_t)(e0 + i) * NN + a] = s.over ? Frame::NO_VALUE : s.result;
        });
    __syncthreads();
    if (lane < ne && g_status[lane] == ROOT_SEARCHED) {
        const size_t e = (size_t)(e0 + lane);
        const bool over = g_over[lane] != 0u;
        const unsigned long long key = g_key[lane];
        value[e] = over ? Frame::NO_VALUE : root_key_value(key, Frame::INF);
        if (best) best[e] = over ? -1 : root_key_square(key);
        if (status) status[e] = (uint8_t)(over ? ROOT_ABORTED : ROOT_SEARCHED);
        if (nodes) nodes[e] = g_nodes[lane];
    }
}

}  // namespace oth_dev
#endif
