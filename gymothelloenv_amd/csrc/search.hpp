// search.hpp -- oth_search: depth-limited alpha-beta over a positional
// evaluation (the spec is the header's comment on oth_search).  V_d(M, O), with
// d discs still to place, is the game end's terminal_weight * (|M| - |O|), at
// d == 0 the evaluation H(M, O) = sum_a weights[a] ([a in M] - [a in O]) +
// mobility_weight (|L(M, O)| - |L(O, M)|), and above the frontier the negamax
// of its children, a pass placing no disc and consuming no depth.
//
// The search is root_tasks.hpp's: a task per root move, the node step built
// from its three blocks, the kernel body and the host driver
// (tests/host/search_host.cpp compiles the part outside __HIPCC__ with g++).
// What differs from solve_step is search_step's leaf rule and the frame:
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
// k_search is root_tasks.hpp's kernel body with the planes built before it.
#pragma once
#include "root_tasks.hpp"

namespace oth {

constexpr int SEARCH_MAX_DEPTH = 14;            // OTH_SEARCH_MAX_DEPTH
constexpr int SEARCH_NO_VALUE = -2147483647 - 1;  // OTH_SEARCH_NO_VALUE
constexpr int SEARCH_INF = 1 << 24;             // every value lies strictly inside (-INF, INF)
constexpr int SEARCH_DONE = ROOT_SEARCHED, SEARCH_TERMINATED = 1, SEARCH_NO_MOVE = 3, SEARCH_ABORTED = ROOT_ABORTED;
constexpr int SEARCH_PLANES = 8;

template <int N>
struct SearchFrame {
    static constexpr int DWORDS = 6 * Geo<N>::W + 3, STACK_DWORDS = (SEARCH_MAX_DEPTH - 1) * DWORDS;
    static constexpr int INF = SEARCH_INF, NO_VALUE = SEARCH_NO_VALUE;
    static OTH_HD void pack(const RootTask<N>& s, uint32_t* f) {
        f[0] = (uint32_t)(s.alpha + SEARCH_INF) | (uint32_t)s.pass << 31;
        f[1] = (uint32_t)(s.beta + SEARCH_INF);
        f[2] = (uint32_t)(s.best + SEARCH_INF);
    }
    static OTH_HD void unpack(RootTask<N>& s, const uint32_t* f) {
        s.alpha = (int)(f[0] & 0x7fffffffu) - SEARCH_INF;
        s.pass = (f[0] >> 31) != 0;
        s.beta = (int)f[1] - SEARCH_INF;
        s.best = (int)f[2] - SEARCH_INF;
    }
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

// One node step of a live task.  depth: the discs the root has to place (>= 1).
template <int N>
OTH_HD void search_step(RootTask<N>& s, uint32_t* st, uint32_t max_nodes, int depth, const SearchEval& ev) {
    constexpr int W = Geo<N>::W;
    if (node_backup<N, SearchFrame<N>>(s, st)) return;
    BB<W> Mn, On;
    if (!node_place<N>(s, max_nodes, Mn, On)) return;
    const bool frontier = s.sp + 1 >= depth;  // the child has no disc left to place
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
        // (never: depth <= SEARCH_MAX_DEPTH; kept for memory safety)
        if (s.sp >= SEARCH_MAX_DEPTH - 1) return task_abandon<N>(s);
        const bool passed = !any(Lc);  // the child's mover has no move: the other side moves again
        return node_descend<N, SearchFrame<N>>(s, st, Mn, On, passed ? Lo : Lc, passed);
    }
    s.best = s.best > v ? s.best : v;
}

// One board on the host (the tests' host build)
template <int N>
inline int search_board_host(const uint64_t* black, const uint64_t* white, const uint64_t* stored, uint32_t meta,
                             int depth, const int8_t* weights, int mobility, int terminal, uint32_t max_nodes,
                             int32_t* value, int32_t* best, int32_t* move_values, uint64_t* nodes) {
    using Board = BB<Geo<N>::W>;
    uint64_t planes[SEARCH_PLANES * Geo<N>::W];
    search_planes<N>(weights, planes);
    const SearchEval ev{planes, mobility, terminal};
    return root_moves_host<N, SearchFrame<N>>(
        black, white, stored, meta,
        [&](const Board& B, const Board& Wt, const Board& Lg, uint32_t m, int& v) {
            return search_status<N>(B, Wt, Lg, m, terminal, v);
        },
        [&](RootTask<N>& s, uint32_t* st) { search_step<N>(s, st, max_nodes, depth, ev); }, value, best,
        move_values, nodes);
}

}  // namespace oth

#if defined(__HIPCC__)

namespace oth_dev {

static_assert(SEARCH_MAX_DEPTH == OTH_SEARCH_MAX_DEPTH && SEARCH_NO_VALUE == OTH_SEARCH_NO_VALUE, "the header's");
static_assert(SEARCH_DONE == OTH_SEARCH_DONE && SEARCH_TERMINATED == OTH_SEARCH_TERMINATED &&
                  SEARCH_NO_MOVE == OTH_SEARCH_NO_MOVE && SEARCH_ABORTED == OTH_SEARCH_ABORTED,
              "the header's status codes");

// the bit-planes of weights + 128 into LDS: lane l holds square 64 k + l, one
// ballot per plane and word.  To be read after a barrier.
template <int N>
__device__ __forceinline__ void build_planes(const int8_t* __restrict__ weights, uint64_t* out) {
    constexpr int W = Geo<N>::W, NN = N * N;
    static_assert(SOLVE_BLOCK == 64, "one ballot is one word of a plane");
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int a = 64 * k + lane;
        const uint32_t u = a < NN ? (uint32_t)((int)weights[a] + 128) : 0u;
#pragma unroll
        for (int b = 0; b < SEARCH_PLANES; ++b) {
            const unsigned long long m = __ballot((u >> b) & 1u);
            if (lane == 0) out[b * W + k] = m;
        }
    }
}

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
    using Board = BB<Geo<N>::W>;
    __shared__ uint64_t g_planes[SEARCH_PLANES * Geo<N>::W];
    build_planes<N>(weights, g_planes);
    const SearchEval ev{g_planes, mobility, terminal};
    root_tasks_kernel<N, SearchFrame<N>>(
        boards, meta, legal, E, value, best, move_values, status, nodes,
        [&](const Board& B, const Board& Wt, const Board& Lg, uint32_t m, int& v) {
            return search_status<N>(B, Wt, Lg, m, terminal, v);
        },
        [&](RootTask<N>& s, uint32_t* st) { search_step<N>(s, st, max_nodes, depth, ev); });
}

}  // namespace oth_dev
#endif
