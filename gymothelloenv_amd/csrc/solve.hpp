// solve.hpp -- oth_solve: exact endgame values and best moves (the spec is the
// header's comment on oth_solve).  G(pos, mover) is the final disc difference
// under best play by both sides, counted from the mover's side, with the
// reference's end-of-game rules (othello.py:424-442, 473-501).
//
// The search is root_tasks.hpp's: a task per root move, the node step built
// from its three blocks, the kernel body and the host driver.  What is the
// solver's own is here:
//   * what a board gets without a search (solve_status);
//   * the frame's packing: every value lies in [-N*N-1, N*N+1], so alpha /
//     beta / best (each + 512, 10 bits) and the pass flag share one dword,
//     FRAME = 6 W + 1 dwords, at most SOLVE_MAX_EMPTIES frames (a pass pushes
//     none, so the depth is at most the empty squares);
//   * the leaf rule of solve_step: the child is a leaf by count (full board,
//     nobody can move), a leaf by the last-ply shortcut (one empty square: the
//     flip count of that square for the child's mover, or else for the other
//     side; no board is updated, no frame pushed), or is descended into.
// tests/host/solve_host.cpp compiles the part outside __HIPCC__ with g++.
#pragma once
#include "root_tasks.hpp"

namespace oth {

constexpr int SOLVE_MAX_EMPTIES = 14;   // OTH_SOLVE_MAX_EMPTIES
constexpr int SOLVE_NO_VALUE = -32768;  // OTH_SOLVE_NO_VALUE
constexpr int SOLVE_EXACT = ROOT_SEARCHED, SOLVE_TERMINATED = 1, SOLVE_SKIPPED = 2, SOLVE_NO_MOVE = 3,
              SOLVE_ABORTED = ROOT_ABORTED;

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

template <int N>
struct SolveFrame {
    static constexpr int DWORDS = 6 * Geo<N>::W + 1, STACK_DWORDS = SOLVE_MAX_EMPTIES * DWORDS;
    static constexpr int INF = N * N + 1, NO_VALUE = SOLVE_NO_VALUE;
    static OTH_HD void pack(const RootTask<N>& s, uint32_t* f) {
        f[0] = (uint32_t)(s.alpha + 512) | (uint32_t)(s.beta + 512) << 10 | (uint32_t)(s.best + 512) << 20 |
               (uint32_t)s.pass << 30;
    }
    static OTH_HD void unpack(RootTask<N>& s, const uint32_t* f) {
        const uint32_t p = f[0];
        s.alpha = (int)(p & 1023u) - 512;
        s.beta = (int)((p >> 10) & 1023u) - 512;
        s.best = (int)((p >> 20) & 1023u) - 512;
        s.pass = ((p >> 30) & 1u) != 0;
    }
};

// One node step of a live task.  levels: the frames the stack holds; a search
// never needs more than the root's empty squares.
template <int N>
OTH_HD void solve_step(RootTask<N>& s, uint32_t* st, uint32_t max_nodes, int levels) {
    constexpr int W = Geo<N>::W, NN = N * N;
    if (node_backup<N, SolveFrame<N>>(s, st)) return;
    BB<W> Mn, On;
    if (!node_place<N>(s, max_nodes, Mn, On)) return;
    const int cm = popcount(Mn), co = popcount(On);
    const int empties = NN - popcount(Mn | On);
    int v = cm - co;  // a leaf by count, from this node's mover's side
    if (empties == 1) {  // the last ply: the flip count of the one square, no board updated
        const int sq = lowest_square<W>(~(Mn | On) & Geo<N>::BOARD);
        const int n1 = popcount(solve_flips<N>(On, Mn, sq));
        if (n1) {
            if (!task_count<N>(s, max_nodes)) return;
            v = cm - co - 1 - 2 * n1;
        } else {
            const int n2 = popcount(solve_flips<N>(Mn, On, sq));
            if (n2) {
                if (!task_count<N>(s, max_nodes)) return;
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
            // (never: levels covers the empty squares; kept for memory safety)
            if (s.sp >= levels) return task_abandon<N>(s);
            return node_descend<N, SolveFrame<N>>(s, st, Mn, On, Lc, passed);
        }
    }
    s.best = s.best > v ? s.best : v;
}

// One board on the host (the tests' host build and the probe's single-thread figure)
template <int N>
inline int solve_board_host(const uint64_t* black, const uint64_t* white, const uint64_t* stored, uint32_t meta,
                            int max_empties, uint32_t max_nodes, int32_t* value, int32_t* best,
                            int32_t* move_values, uint64_t* nodes) {
    using Board = BB<Geo<N>::W>;
    return root_moves_host<N, SolveFrame<N>>(
        black, white, stored, meta,
        [&](const Board& B, const Board& Wt, const Board& Lg, uint32_t m, int& v) {
            return solve_status<N>(B, Wt, Lg, m, max_empties, v);
        },
        [&](RootTask<N>& s, uint32_t* st) { solve_step<N>(s, st, max_nodes, max_empties); }, value, best,
        move_values, nodes);
}

}  // namespace oth

#if defined(__HIPCC__)

namespace oth_dev {

static_assert(SOLVE_MAX_EMPTIES == OTH_SOLVE_MAX_EMPTIES && SOLVE_NO_VALUE == OTH_SOLVE_NO_VALUE, "the header's");
static_assert(SOLVE_EXACT == OTH_SOLVE_EXACT && SOLVE_TERMINATED == OTH_SOLVE_TERMINATED &&
                  SOLVE_SKIPPED == OTH_SOLVE_SKIPPED && SOLVE_NO_MOVE == OTH_SOLVE_NO_MOVE &&
                  SOLVE_ABORTED == OTH_SOLVE_ABORTED,
              "the header's status codes");

template <int N>
__global__ __launch_bounds__(SOLVE_BLOCK) void k_solve(const uint64_t* __restrict__ boards,
                                                       const uint16_t* __restrict__ meta,
                                                       const uint64_t* __restrict__ legal, int E, int max_empties,
                                                       uint32_t max_nodes, int32_t* __restrict__ value,
                                                       int32_t* __restrict__ best, int32_t* __restrict__ move_values,
                                                       uint8_t* __restrict__ status,
                                                       unsigned long long* __restrict__ nodes) {
    using Board = BB<Geo<N>::W>;
    root_tasks_kernel<N, SolveFrame<N>>(
        boards, meta, legal, E, value, best, move_values, status, nodes,
        [&](const Board& B, const Board& Wt, const Board& Lg, uint32_t m, int& v) {
            return solve_status<N>(B, Wt, Lg, m, max_empties, v);
        },
        [&](RootTask<N>& s, uint32_t* st) { solve_step<N>(s, st, max_nodes, max_empties); });
}

}  // namespace oth_dev
#endif
