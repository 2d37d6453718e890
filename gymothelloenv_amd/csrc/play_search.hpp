// play_search.hpp -- the search as a player: oth_play_search (oth_step_policy
// with the mover's move chosen by oth_search's computation, a configuration per
// colour) and oth_reset_vs_search / oth_step_vs_search (oth_reset_vs /
// oth_step_vs with the embedded opponent's move chosen so).  The spec is the
// header's comment on oth_play_search.
//
// The searched move S(board, cfg): with e empty squares the search runs to
// depth d = e when e <= cfg.endgame (every line then reaches a game end: the
// move is oth_solve's), else to cfg.depth; a finished search plays its best
// move, a search over its budget plays GreedyPolicy's move (the most flips, the
// lowest square of equals) and the ply counts as a fallback.
//
// The shared core (the part outside __HIPCC__: the depth rule, the greedy key
// by solve_flips popcounts and one board's move on the host) is plain host /
// device code: tests/host/play_search_host.cpp compiles the same text with g++.
//
// Device mapping (k_play_search): root_tasks.hpp's run_tasks (a block of one
// wave over SOLVE_GROUP boards, a lane per (board, root move) task, the tasks
// packed over the lanes in 64-task chunks) over search_step, the tasks loaded
// from LDS, the best move / over-budget reduced there with root_key, in rounds:
//   * the lanes < SOLVE_GROUP own their boards' Lane<N> state in registers for
//     the whole call.  In a round every owner advances its board through
//     everything that needs no search (the protagonist's ply, random-opening
//     plies, a terminated board's plies, tallies, auto-reset: a per-board phase
//     that only moves forward) until the board wants a searched move or is
//     finished for this call, and publishes (mover, opponent, move mask, depth,
//     which side's evaluation) to LDS;
//   * after a barrier the wave reads the group's task count from LDS -- the
//     loop's exit test is block-uniform -- and leaves when there is none;
//   * otherwise it searches every task (depth, evaluation and budget per task:
//     boards in endgame mode sit beside boards in depth mode, black movers
//     beside white ones), reduces, and the owners apply S through step_lane.
// Every round places a disc on every wanting board or finishes it, the rounds
// are bounded by n_plies (play) or the board's phase sequence (vs), and every
// search by max_nodes.
#pragma once
#include "search.hpp"

namespace oth {

// one colour's oth_search_policy as the kernel takes it (weights: device memory on the device)
struct PlaySearchSide {
    const int8_t* weights;
    int depth, mobility, terminal, endgame;
    uint32_t max_nodes;
};

// the discs the root places: all of them from `endgame` empty squares on (at least one: a board that is searched has a move)
OTH_HD int play_search_depth(int empties, int depth, int endgame) {
    const int d = empties <= endgame ? empties : depth;
    return d < 1 ? 1 : d;
}

// GreedyPolicy's order on root moves (simple_policies.py:69-92): the max of
// (flips << 8 | 255 - square) is the lowest square of the most flips
template <int N>
OTH_HD int play_search_flip_key(const BB<Geo<N>::W>& mover, const BB<Geo<N>::W>& opp, int a) {
    return popcount(solve_flips<N>(mover, opp, a)) << 8 | (255 - a);
}

// S of one board on the host (the tests' host build): the move, -1 for a
// terminated board and for a live one whose stored possible_moves is empty
// (GreedyPolicy's None); *fallback: the search ran over its budget.
template <int N>
inline int play_search_move_host(const uint64_t* black, const uint64_t* white, const uint64_t* stored, uint32_t meta,
                                 const PlaySearchSide& c, int* fallback) {
    constexpr int W = Geo<N>::W, NN = N * N;
    static_assert(NN <= 256, "a square fits the key's low byte");
    BB<W> B, Wt, Lg;
    for (int i = 0; i < W; ++i) {
        B.w[i] = black[i];
        Wt.w[i] = white[i];
        Lg.w[i] = stored[i];
    }
    *fallback = 0;
    int v0;
    if (search_status<N>(B, Wt, Lg, meta, c.terminal, v0) != SEARCH_DONE) return -1;
    const int d = play_search_depth(NN - popcount(B | Wt), c.depth, c.endgame);
    int32_t value, best, mv[NN];
    uint64_t nodes;
    const int st = search_board_host<N>(black, white, stored, meta, d, c.weights, c.mobility, c.terminal, c.max_nodes,
                                        &value, &best, mv, &nodes);
    if (st == SEARCH_DONE) return best;
    *fallback = 1;
    const bool tw = (meta & 1u) != 0;
    const BB<W> mover = tw ? Wt : B, opp = tw ? B : Wt;
    BB<W> todo = Lg & Geo<N>::BOARD;
    int key = 0;
    while (any(todo)) {
        const int a = lowest_square<W>(todo);
        todo = todo & ~square<W>(a);
        const int k = play_search_flip_key<N>(mover, opp, a);
        key = k > key ? k : key;
    }
    return 255 - (key & 255);
}

}  // namespace oth

#if defined(__HIPCC__)
#include "play_owner.hpp"

namespace oth_dev {

// MODE PS_PLAY: side_b is black's policy, side_w white's, ctr the first ply's counter; the vs modes: both are
// the opponent's, ctr the call's counter.  same: both sides read one weight table (one plane set is built).
// Outputs: actions / rewards / dones / fb_ply [n_plies][E] in play mode; rewards / dones / plies_out / fb_cnt [E]
// in PS_STEP_VS; none in PS_RESET_VS (mask: the boards to reset, NULL for all).  Each may be NULL.
template <int N, int MODE>
__global__ __launch_bounds__(SOLVE_BLOCK) void k_play_search(
    uint64_t* __restrict__ boards, uint16_t* __restrict__ meta, uint64_t* __restrict__ legal, int E, uint32_t flags,
    PlaySearchSide side_b, PlaySearchSide side_w, int same, int n_plies, const int32_t* __restrict__ act_in,
    const int8_t* __restrict__ prot, const uint8_t* __restrict__ mask, int32_t* __restrict__ actions,
    int32_t* __restrict__ rewards, uint8_t* __restrict__ dones, uint8_t* __restrict__ fb_ply,
    int32_t* __restrict__ plies_out, int32_t* __restrict__ fb_cnt, unsigned long long* __restrict__ wdl,
    unsigned long long* __restrict__ wdl_vs, Rng rng, uint64_t ctr) {
    constexpr int W = Geo<N>::W, NN = N * N, G = SOLVE_GROUP;
    static_assert(NN <= 256, "a square fits the reduction keys' low byte");
    __shared__ uint64_t g_planes[2][SEARCH_PLANES * W];
    __shared__ uint64_t g_M[G][W], g_O[G][W], g_moves[G][W];  // a wanting board's mover, opponent and root moves
    __shared__ int g_cnt[G];    // its tasks; 0: the board wants no search this round
    __shared__ int g_depth[G], g_side[G];
    __shared__ unsigned long long g_key[G];  // max of root_key
    __shared__ int g_gkey[G];                // max of play_search_flip_key: the fallback's move
    __shared__ unsigned int g_over[G];
    ctr += *rng.ply_off;  // graph-region offset (oth_graph_end); 0 eagerly
    const int lane = threadIdx.x;
    const long long e0 = (long long)blockIdx.x * G;
    const int ne = (int)(E - e0 < G ? E - e0 : G);
    build_planes<N>(side_b.weights, g_planes[0]);  // the evaluation's planes per colour
    if (!same) build_planes<N>(side_w.weights, g_planes[1]);  // (same: a kernel argument, uniform)
    const uint64_t* planes_w = same ? g_planes[0] : g_planes[1];

    // ---- the owners' state and control flow (play_owner.hpp)
    PlayOwner<N, MODE> o;
    o.init(MODE, lane, e0, ne, boards, meta, legal, E, flags, n_plies, act_in, prot, mask, actions, rewards, dones,
           fb_ply, rng, ctr);
    const Lane<N>& s = o.s;
    if (lane < G) {
#pragma unroll
        for (int k = 0; k < W; ++k) g_M[lane][k] = g_O[lane][k] = g_moves[lane][k] = 0ull;
        g_depth[lane] = 1;
        g_side[lane] = 0;
    }

    // ---- the rounds
    for (;;) {
        bool want = false;
        if (lane < G) {
            if (o.owner) want = o.advance();
            int cnt = 0;
            if (want) {
                const bool tw = (s.meta & M_TURN_WHITE) != 0;
                const BB<W> M = pick(tw, s.white, s.black), O = pick(tw, s.black, s.white);
                const BB<W> mv = s.legal & Geo<N>::BOARD;
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    g_M[lane][k] = M.w[k];
                    g_O[lane][k] = O.w[k];
                    g_moves[lane][k] = mv.w[k];
                }
                const bool sw = MODE == PS_PLAY && tw;
                g_side[lane] = sw ? 1 : 0;
                g_depth[lane] = play_search_depth(NN - popcount(M | O), sw ? side_w.depth : side_b.depth,
                                                  sw ? side_w.endgame : side_b.endgame);
                cnt = popcount(mv);
            }
            g_cnt[lane] = cnt;
            g_key[lane] = 0ull;
            g_gkey[lane] = 0;
            g_over[lane] = 0u;
        }
        __syncthreads();
        // the tasks: depth, evaluation and budget are their board's.  The count is read from LDS after the
        // barrier: the exit test is block-uniform
        const int total = run_tasks<N, SearchFrame<N>>(
            g_moves, g_cnt,
            [&](int i, int a, bool active, BB<W>& M, BB<W>& O) {
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    M.w[k] = g_M[i][k];
                    O.w[k] = g_O[i][k];
                }
                if (active) atomicMax(&g_gkey[i], play_search_flip_key<N>(M, O, a));
                const bool sw = g_side[i] != 0;
                const int depth = g_depth[i];
                const uint32_t max_nodes = sw ? side_w.max_nodes : side_b.max_nodes;
                const SearchEval ev{sw ? planes_w : g_planes[0], sw ? side_w.mobility : side_b.mobility,
                                    sw ? side_w.terminal : side_b.terminal};
                return [=](RootTask<N>& s, uint32_t* st) { search_step<N>(s, st, max_nodes, depth, ev); };
            },
            [&](const RootTask<N>& s, int i, int a) {
                if (s.over) atomicOr(&g_over[i], 1u);
                else atomicMax(&g_key[i], root_key(s.result, SEARCH_INF, a));
            });
        if (total == 0) break;
        __syncthreads();
        if (want) {
            const bool over = g_over[lane] != 0u;
            o.apply(over ? 255 - (g_gkey[lane] & 255) : root_key_square(g_key[lane]), over ? 1 : 0);
        }
    }

    // ---- the boards back, the call's outputs, the tallies: two blocks share a W/D/L slot (the handle has one
    // per 16 boards)
    o.finish(boards, meta, legal, plies_out, fb_cnt, wdl, wdl_vs, (size_t)(blockIdx.x >> 1));
}

}  // namespace oth_dev
#endif
