// search.hpp -- oth_search: depth-limited alpha-beta over a positional
// evaluation (the spec is the header's comment on oth_search).  V_d(M, O), with
// d discs still to place, is the game end's terminal_weight * (|M| - |O|), at
// d == 0 the evaluation H(M, O) = sum_a weights[a] ([a in M] - [a in O]) +
// mobility_weight (|L(M, O)| - |L(O, M)|), and above the frontier the negamax
// of its children, a pass placing no disc and consuming no depth.
//
// The search core (the part outside __HIPCC__) is solve.hpp's node-step negamax
// with its pieces (solve_flips, solve_legal, lowest_square, the task, the array
// stack, the budget count): tests/host/search_host.cpp compiles the same text
// with g++.  What differs from solve_step:
//   * the depth: the root pseudo-node is level 0 and a pass pushes no frame, so
//     a node at level sp has depth - sp discs to place and the stack holds at
//     most depth - 1 frames;
//   * a child with no disc left to place is a leaf: the game end's value if
//     neither side can move (rule 1 comes before rule 2), else H.  There is no
//     last-ply shortcut: every placement is one node;
//   * the values.  |H| <= 128 * 256 + 127 * 256 < 2^16 and |T| <= 32767 * 256 <
//     2^23, so every value lies strictly inside (-2^24, 2^24) = (-INF, INF),
//     and alpha / beta / best, in [-INF, INF], take a dword each in the frame
//     (+ INF, 26 bits; the pass flag rides in alpha's dword): FRAME = 6 W + 3.
//
// The evaluation does not loop over squares.  Eight bit-planes of weights[a] +
// 128 (plane b holds the squares whose biased weight has bit b set; W words
// each) turn the weighted sum of a set X into
//     sum_b 2^b popcount(X & plane_b) - 128 popcount(X):
// 8 W popcounts per side whatever the weights.  The block builds the planes
// once into LDS (one ballot per plane and word) and every lane reads the same
// address: a broadcast.
//
// Device mapping (k_search): k_solve's.  One lane per (board, root move) task,
// a block of one wave per SOLVE_GROUP boards, the tasks packed over the lanes
// in 64-task chunks, value / best / status / nodes reduced in LDS; the key of
// the max is 64 bits wide here.  The stack is the per-lane array (scratch).
#pragma once
#include "solve.hpp"

namespace oth {

constexpr int SEARCH_MAX_DEPTH = 14;            // OTH_SEARCH_MAX_DEPTH
constexpr int SEARCH_NO_VALUE = -2147483647 - 1;  // OTH_SEARCH_NO_VALUE
constexpr int SEARCH_INF = 1 << 24;             // every value lies strictly inside (-INF, INF)
constexpr int SEARCH_DONE = 0, SEARCH_TERMINATED = 1, SEARCH_NO_MOVE = 3, SEARCH_ABORTED = 4;
constexpr int SEARCH_PLANES = 8;

template <int N>
struct SearchFrame {
    static constexpr int W = Geo<N>::W;
    static constexpr int DWORDS = 6 * W + 3;
};

// The evaluation's constants: planes[b * W + k] is word k of bit-plane b.
struct SearchEval {
    const uint64_t* planes;
    int mobility, terminal;
};

// word k of bit-plane b of weights + 128 (the host build; the device builds them by ballots)
template <int N>
inline void search_planes(const int8_t* weights, uint64_t* planes) {
    constexpr int W = Geo<N>::W, NN = N * N;
    for (int i = 0; i < SEARCH_PLANES * W; ++i) planes[i] = 0;
    for (int a = 0; a < NN; ++a) {
        const uint32_t u = (uint32_t)((int)weights[a] + 128);
        for (int b = 0; b < SEARCH_PLANES; ++b)
            if ((u >> b) & 1u) planes[b * W + a / 64] |= 1ull << (a % 64);
    }
}

// sum_a weights[a] ([a in M] - [a in O])
template <int N>
OTH_HD int search_weighted(const BB<Geo<N>::W>& M, const BB<Geo<N>::W>& O, const uint64_t* planes) {
    constexpr int W = Geo<N>::W;
    int sum = -128 * (popcount(M) - popcount(O));
#pragma unroll
    for (int b = 0; b < SEARCH_PLANES; ++b) {
        int c = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const uint64_t p = planes[b * W + k];
            c += popc64(M.w[k] & p) - popc64(O.w[k] & p);
        }
        sum += c * (1 << b);
    }
    return sum;
}

// What a board gets without a search: its status and, for a terminated board, its value.
template <int N>
OTH_HD int search_status(const BB<Geo<N>::W>& black, const BB<Geo<N>::W>& white, const BB<Geo<N>::W>& stored,
                         uint32_t meta, int terminal, int& value) {
    value = SEARCH_NO_VALUE;
    if (meta & 2u) {  // terminated: the discs of the side in the turn bit minus the other's
        const int nb = popcount(black), nw = popcount(white);
        value = terminal * ((meta & 1u) ? nw - nb : nb - nw);
        return SEARCH_TERMINATED;
    }
    if (!any(stored & Geo<N>::BOARD)) return SEARCH_NO_MOVE;
    return SEARCH_DONE;
}

// the task of root move a: a pseudo-node with that one move and the full window
template <int N>
OTH_HD void search_task_init(SolveTask<N>& s, const BB<Geo<N>::W>& mover, const BB<Geo<N>::W>& opp, int a) {
    solve_task_init<N>(s, mover, opp, a);
    s.alpha = -SEARCH_INF;
    s.beta = SEARCH_INF;
    s.best = -SEARCH_INF;
}

template <int N, typename Stack>
OTH_HD void search_push(const SolveTask<N>& s, Stack& st) {
    constexpr int W = Geo<N>::W, F = SearchFrame<N>::DWORDS;
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
    st.put(at + 6 * W + 0, (uint32_t)(s.alpha + SEARCH_INF) | (uint32_t)s.pass << 31);
    st.put(at + 6 * W + 1, (uint32_t)(s.beta + SEARCH_INF));
    st.put(at + 6 * W + 2, (uint32_t)(s.best + SEARCH_INF));
}

template <int N, typename Stack>
OTH_HD void search_pop(SolveTask<N>& s, const Stack& st) {
    constexpr int W = Geo<N>::W, F = SearchFrame<N>::DWORDS;
    const int at = s.sp * F;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        s.M.w[i] = (uint64_t)st.get(at + 6 * i + 1) << 32 | st.get(at + 6 * i + 0);
        s.O.w[i] = (uint64_t)st.get(at + 6 * i + 3) << 32 | st.get(at + 6 * i + 2);
        s.R.w[i] = (uint64_t)st.get(at + 6 * i + 5) << 32 | st.get(at + 6 * i + 4);
    }
    const uint32_t p = st.get(at + 6 * W);
    s.alpha = (int)(p & 0x7fffffffu) - SEARCH_INF;
    s.pass = (p >> 31) != 0;
    s.beta = (int)st.get(at + 6 * W + 1) - SEARCH_INF;
    s.best = (int)st.get(at + 6 * W + 2) - SEARCH_INF;
}

// One node step of a live task.  depth: the discs the root has to place (>= 1).
template <int N, typename Stack>
OTH_HD void search_step(SolveTask<N>& s, Stack& st, uint32_t max_nodes, int depth, const SearchEval& ev) {
    constexpr int W = Geo<N>::W;
    if (!any(s.R) || s.best >= s.beta) {  // the node is finished: back up one level
        const int v = s.pass ? -s.best : s.best;
        if (s.sp == 0) {
            s.result = v;
            s.live = false;
            return;
        }
        --s.sp;
        search_pop<N>(s, st);
        s.best = s.best > -v ? s.best : -v;
        if (!any(s.R) || s.best >= s.beta) return;  // the parent is finished too: the next step's
    }
    if (!solve_count<N>(s, max_nodes)) return;
    const int a = lowest_square<W>(s.R);
    const BB<W> bit = square<W>(a);
    s.R = s.R & ~bit;
    const BB<W> fl = solve_flips<N>(s.M, s.O, a);
    const BB<W> Mn = s.M | fl | bit, On = s.O & ~fl;  // the child: On to move against Mn
    const bool frontier = s.sp + 1 >= depth;          // the child has no disc left to place
    const BB<W> Lc = solve_legal<N>(On, Mn);
    BB<W> Lo = zero<W>();
    // the other side's scan: the game-end test's when the child's mover has no
    // move, the mobility term's at the frontier (skipped where its weight is 0)
    if (!any(Lc) || (frontier && ev.mobility != 0)) Lo = solve_legal<N>(Mn, On);
    int v;  // a leaf's value, from this node's mover's side
    if (!any(Lc) && !any(Lo)) {
        v = ev.terminal * (popcount(Mn) - popcount(On));
    } else if (frontier) {
        v = search_weighted<N>(Mn, On, ev.planes) + ev.mobility * (popcount(Lo) - popcount(Lc));
    } else {
        if (s.sp >= SEARCH_MAX_DEPTH - 1) {  // (never: depth <= SEARCH_MAX_DEPTH; kept for memory safety)
            s.over = true;
            s.live = false;
            return;
        }
        const bool passed = !any(Lc);  // the child's mover has no move: the other side moves again
        search_push<N>(s, st);
        ++s.sp;
        const int lo = s.alpha > s.best ? s.alpha : s.best;
        s.alpha = passed ? lo : -s.beta;  // the child's window is (-beta, -lo); a pass negates it again
        s.beta = passed ? s.beta : -lo;
        s.best = -SEARCH_INF;
        s.pass = passed;
        s.M = passed ? Mn : On;
        s.O = passed ? On : Mn;
        s.R = passed ? Lo : Lc;
        return;
    }
    s.best = s.best > v ? s.best : v;
}

// the stack of one task: depth - 1 frames at most
template <int N>
using SearchStack = SolveArrayStack<(SEARCH_MAX_DEPTH - 1) * SearchFrame<N>::DWORDS>;

// One board on the host (the tests' host build): the spec's outputs for one
// board, the tasks in ascending squares.  move_values: N*N entries.  Returns the status.
template <int N>
inline int search_board_host(const uint64_t* black, const uint64_t* white, const uint64_t* stored, uint32_t meta,
                             int depth, const int8_t* weights, int mobility, int terminal, uint32_t max_nodes,
                             int32_t* value, int32_t* best, int32_t* move_values, uint64_t* nodes) {
    constexpr int W = Geo<N>::W, NN = N * N;
    BB<W> B, Wt, Lg;
    for (int i = 0; i < W; ++i) {
        B.w[i] = black[i];
        Wt.w[i] = white[i];
        Lg.w[i] = stored[i];
    }
    for (int a = 0; a < NN; ++a) move_values[a] = SEARCH_NO_VALUE;
    *best = -1;
    *nodes = 0;
    int v0;
    const int status = search_status<N>(B, Wt, Lg, meta, terminal, v0);
    *value = v0;
    if (status != SEARCH_DONE) return status;
    uint64_t planes[SEARCH_PLANES * W];
    search_planes<N>(weights, planes);
    const SearchEval ev{planes, mobility, terminal};
    const bool tw = (meta & 1u) != 0;
    const BB<W> mover = tw ? Wt : B, opp = tw ? B : Wt;
    BB<W> todo = Lg & Geo<N>::BOARD;
    bool aborted = false;
    int bv = -SEARCH_INF, ba = -1;
    SearchStack<N> st;
    while (any(todo)) {
        const int a = lowest_square<W>(todo);
        todo = todo & ~square<W>(a);
        SolveTask<N> s;
        search_task_init<N>(s, mover, opp, a);
        while (s.live) search_step<N>(s, st, max_nodes, depth, ev);
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
    if (aborted) return SEARCH_ABORTED;
    *value = bv;
    *best = ba;
    return SEARCH_DONE;
}

}  // namespace oth

#if defined(__HIPCC__)

namespace oth_dev {

static_assert(SEARCH_MAX_DEPTH == OTH_SEARCH_MAX_DEPTH && SEARCH_NO_VALUE == OTH_SEARCH_NO_VALUE, "the header's");
static_assert(SEARCH_DONE == OTH_SEARCH_DONE && SEARCH_TERMINATED == OTH_SEARCH_TERMINATED &&
                  SEARCH_NO_MOVE == OTH_SEARCH_NO_MOVE && SEARCH_ABORTED == OTH_SEARCH_ABORTED,
              "the header's status codes");

template <int N>
__global__ __launch_bounds__(SOLVE_BLOCK) void k_search(const uint64_t* __restrict__ boards,
                                                        const uint16_t* __restrict__ meta,
                                                        const uint64_t* __restrict__ legal, int E, int depth,
                                                        const int8_t* __restrict__ weights, int mobility,
                                                        int terminal, uint32_t max_nodes,
                                                        int32_t* __restrict__ value, int32_t* __restrict__ best,
                                                        int32_t* __restrict__ move_values,
                                                        uint8_t* __restrict__ status,
                                                        unsigned long long* __restrict__ nodes) {
    constexpr int W = Geo<N>::W, NN = N * N, G = SOLVE_GROUP;
    static_assert(NN <= 256, "a square fits the reduction key's low byte");
    static_assert(SOLVE_BLOCK == 64, "one ballot is one word of a plane");
    __shared__ uint64_t g_planes[SEARCH_PLANES * W];
    __shared__ uint64_t g_moves[G][W];  // the searched boards' stored possible_moves; none for the others
    __shared__ int g_cnt[G];
    __shared__ unsigned long long g_key[G];  // max of (value + INF) << 8 | (255 - square): the lowest square of the best value
    __shared__ unsigned int g_over[G];
    __shared__ unsigned long long g_nodes[G];
    __shared__ int g_status[G];
    const int lane = threadIdx.x;
    const long long e0 = (long long)blockIdx.x * G;
    const int ne = (int)(E - e0 < G ? E - e0 : G);
    if (lane < G) {
        BB<W> mv = zero<W>();
        int st = SEARCH_NO_MOVE;
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
            st = search_status<N>(B, Wt, Lg, meta[e], terminal, v);
            if (st == SEARCH_DONE) {
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
    // the bit-planes of weights + 128: lane l holds square 64 k + l, one ballot per plane
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int a = 64 * k + lane;
        const uint32_t u = a < NN ? (uint32_t)((int)weights[a] + 128) : 0u;
#pragma unroll
        for (int b = 0; b < SEARCH_PLANES; ++b) {
            const unsigned long long m = __ballot((u >> b) & 1u);
            if (lane == 0) g_planes[b * W + k] = m;
        }
    }
    __syncthreads();
    const SearchEval ev{g_planes, mobility, terminal};
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
            if (!test(mv, a)) move_values[(size_t)(e0 + i) * NN + a] = SEARCH_NO_VALUE;
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
        search_task_init<N>(s, pick(tw, Wt, B), pick(tw, B, Wt), a);
        s.live = active;
        SearchStack<N> st;
        while (__any(s.live))
            if (s.live) search_step<N>(s, st, max_nodes, depth, ev);
        if (active) {
            if (s.over) atomicOr(&g_over[i], 1u);
            else atomicMax(&g_key[i], (unsigned long long)(s.result + SEARCH_INF) << 8 | (unsigned long long)(255 - a));
            atomicAdd(&g_nodes[i], (unsigned long long)s.nodes + (s.over ? 1ull : 0ull));
            if (move_values) move_values[e * NN + a] = s.over ? SEARCH_NO_VALUE : s.result;
        }
    }
    __syncthreads();
    if (lane < ne && g_status[lane] == SEARCH_DONE) {
        const size_t e = (size_t)(e0 + lane);
        const bool over = g_over[lane] != 0u;
        const unsigned long long key = g_key[lane];
        value[e] = over ? SEARCH_NO_VALUE : (int)(key >> 8) - SEARCH_INF;
        if (best) best[e] = over ? -1 : 255 - (int)(key & 255ull);
        if (status) status[e] = (uint8_t)(over ? SEARCH_ABORTED : SEARCH_DONE);
        if (nodes) nodes[e] = g_nodes[lane];
    }
}

}  // namespace oth_dev
#endif
