// play_ntuple.hpp -- the n-tuple network as a player: oth_play_ntuple (oth_play_search with the
// mover's move chosen by oth_search_ntuple's computation, a policy per colour, an exploring draw
// before the search, and the TD(0) rows of the plies from the same launch) and
// oth_reset_vs_ntuple / oth_step_vs_ntuple (the embedded opponent's move chosen so).  The spec is
// the header's comment on oth_ntuple_policy.
//
// The move T(board, p): play_search.hpp's S with ntuple_search_step in place of search_step -- the
// depth rule, the stored root list, `best` of a finished search, GreedyPolicy's move and a fallback
// for one over its budget -- after the exploring draw: x = philox4(seed, id, g, 8); the ply explores
// iff (x.x >> 16) < explore, and then plays the floor(x.y count / 2^32)-th square of the stored mask.
//
// The target of a learning row: the position after the move, before any auto-reset, seen from the
// row's mover under the mover's own policy -- 32768 sign(disc difference) at a game end, +H of the
// next row where the same side moves again (a pass), -H otherwise.
//
// The shared core (the part outside __HIPCC__: the draw, T of one board and the target rule) is
// plain host / device code: tests/host/play_ntuple_host.cpp compiles the same text with g++.
//
// Device mapping (k_play_ntuple): k_play_search's, round for round -- a wave per SOLVE_GROUP boards,
// the owners in the lanes < SOLVE_GROUP (play_owner.hpp), run_tasks over ntuple_search_step with the
// task's side selecting plan, weights, depth, terminal and budget, the greedy key reduced in LDS.
// Both plans sit in LDS (at most 2 x 2,336 bytes), the weights stay in global memory.  An owner whose
// ply explores applies the drawn move and advances again inside the round, so a round still places a
// searched disc on every wanting board.  With td rows the block zero-fills its boards' slices first;
// after a round's search the wave forms the targets of the boards that learn as k_ntuple_eval forms
// a value -- eight lanes a board, lane s taking symmetry s, three xor shuffles -- and the owners store
// the rows before they apply the move.
#pragma once
#include "ntuple.hpp"
#include "play_search.hpp"

namespace oth {

constexpr uint32_t NTUPLE_EXPLORE_PURPOSE = 8u;  // the draw's Philox purpose (state.hpp RNG_NTUPLE_EXPLORE)
constexpr int NTUPLE_EXPLORE_ONE = 65536;        // OTH_NTUPLE_EXPLORE_ONE
constexpr int NTUPLE_PLAN_WORDS = NTUPLE_HEAD + NTUPLE_REC * NTUPLE_MAX_TUPLES;

// one colour's oth_ntuple_policy as the kernel takes it (plan: LDS on the device; weights: device memory there)
struct PlayNtupleSide {
    const uint32_t* plan;
    const int32_t* weights;
    int depth, terminal, endgame, explore;
    uint32_t max_nodes;
};

// The exploring draw of ply g of board id over a stored mask of `count` squares (count >= 1): true
// and k, the index of the move in ascending squares.  explore = 0 never draws.
OTH_HD bool ntuple_explores(uint64_t seed, uint32_t id, uint64_t g, int explore, int count, int& k) {
    if (explore <= 0) return false;
    const U4 x = philox4(seed, id, g, NTUPLE_EXPLORE_PURPOSE);
    if ((x.x >> 16) >= (uint32_t)explore) return false;
    k = (int)(((uint64_t)x.y * (uint64_t)(uint32_t)count) >> 32);
    return true;
}

// what a move leaves: the game is over, the other side is to move, or the mover moves again (a pass)
constexpr int TD_OVER = 0, TD_TURN = 1, TD_PASS = 2;

// The position after M places a disc on a against O (Mn, On: the same sides afterwards) and which of the three it is
template <int N>
OTH_HD int ntuple_td_after(const BB<Geo<N>::W>& M, const BB<Geo<N>::W>& O, int a, BB<Geo<N>::W>& Mn, BB<Geo<N>::W>& On) {
    constexpr int W = Geo<N>::W;
    const BB<W> bit = square<W>(a), fl = solve_flips<N>(M, O, a);
    Mn = M | fl | bit;
    On = O & ~fl;
    if (any(solve_legal<N>(On, Mn))) return TD_TURN;
    return any(solve_legal<N>(Mn, On)) ? TD_PASS : TD_OVER;
}

// the target from the mover's side: diff its discs minus the opponent's after the move, h the value
// of the next row from the side to move there
OTH_HD int32_t ntuple_td_value(int kind, int diff, int32_t h) {
    if (kind == TD_OVER) return NTUPLE_VALUE_ONE * ((diff > 0) - (diff < 0));
    return kind == TD_PASS ? h : -h;
}

// the target of one row on the host: M moves on a against O under the plan and the weights
template <int N>
inline int32_t play_ntuple_target_host(const BB<Geo<N>::W>& M, const BB<Geo<N>::W>& O, int a, const uint32_t* plan,
                                       const int32_t* weights) {
    constexpr int W = Geo<N>::W;
    BB<W> Mn, On;
    const int kind = ntuple_td_after<N>(M, O, a, Mn, On);
    int32_t h = 0;
    if (kind == TD_TURN) h = ntuple_value(ntuple_sum(plan, weights, On.w, Mn.w), (int)plan[3]);
    if (kind == TD_PASS) h = ntuple_value(ntuple_sum(plan, weights, Mn.w, On.w), (int)plan[3]);
    return ntuple_td_value(kind, popcount(Mn) - popcount(On), h);
}

// T of one board on the host (the tests' host build): the move, -1 for a terminated board and for
// a live one whose stored possible_moves is empty; *fallback: the search ran over its budget;
// *explored: the ply explored (no search); *target (may be NULL): the row's target where the move
// is a finished search's, else 0.
template <int N>
inline int play_ntuple_move_host(const uint64_t* black, const uint64_t* white, const uint64_t* stored, uint32_t meta,
                                 const PlayNtupleSide& c, uint64_t seed, uint32_t id, uint64_t g, int* fallback,
                                 int* explored, int32_t* target) {
    constexpr int W = Geo<N>::W, NN = N * N;
    static_assert(NN <= 256, "a square fits the key's low byte");
    BB<W> B, Wt, Lg;
    for (int i = 0; i < W; ++i) {
        B.w[i] = black[i];
        Wt.w[i] = white[i];
        Lg.w[i] = stored[i];
    }
    *fallback = 0;
    *explored = 0;
    if (target) *target = 0;
    int v0;
    if (search_status<N>(B, Wt, Lg, meta, c.terminal, v0) != SEARCH_DONE) return -1;
    const BB<W> mv = Lg & Geo<N>::BOARD;
    int k;
    if (ntuple_explores(seed, id, g, c.explore, popcount(mv), k)) {
        *explored = 1;
        return select_bit<W>(mv, k);
    }
    const bool tw = (meta & 1u) != 0;
    const BB<W> mover = tw ? Wt : B, opp = tw ? B : Wt;
    const int d = play_search_depth(NN - popcount(B | Wt), c.depth, c.endgame);
    int32_t value, best, move_values[NN];
    uint64_t nodes;
    const int st = ntuple_search_board_host<N>(black, white, stored, meta, d, c.plan, c.weights, c.terminal, c.max_nodes,
                                               &value, &best, move_values, &nodes);
    if (st == SEARCH_DONE) {
        if (target) *target = play_ntuple_target_host<N>(mover, opp, best, c.plan, c.weights);
        return best;
    }
    *fallback = 1;
    BB<W> todo = mv;
    int key = 0;
    while (any(todo)) {
        const int a = lowest_square<W>(todo);
        todo = todo & ~square<W>(a);
        const int kk = play_search_flip_key<N>(mover, opp, a);
        key = kk > key ? kk : key;
    }
    return 255 - (key & 255);
}

}  // namespace oth

#if defined(__HIPCC__)
#include "play_owner.hpp"

namespace oth_dev {

static_assert(RNG_NTUPLE_EXPLORE == NTUPLE_EXPLORE_PURPOSE, "one purpose word");

// struct oth_ntuple_td as the kernel takes it: all four NULL without td rows
struct PlayNtupleTd {
    uint64_t* boards;
    uint16_t* meta;
    int32_t* targets;
    uint8_t* learn;
};

// MODE PS_PLAY: side_b is black's policy, side_w white's (their plan: the device copy), ctr the first ply's
// counter; the vs modes: both are the opponent's, ctr the call's counter.  same: both sides read one plan (one
// copy is made).  Outputs: k_play_search's; td (play mode only): [n_plies][E] rows.
template <int N, int MODE>
__global__ __launch_bounds__(SOLVE_BLOCK) void k_play_ntuple(
    uint64_t* __restrict__ boards, uint16_t* __restrict__ meta, uint64_t* __restrict__ legal, int E, uint32_t flags,
    PlayNtupleSide side_b, PlayNtupleSide side_w, NtupleKey key_b, NtupleKey key_w, int same, int n_plies,
    const int32_t* __restrict__ act_in, const int8_t* __restrict__ prot, const uint8_t* __restrict__ mask,
    int32_t* __restrict__ actions, int32_t* __restrict__ rewards, uint8_t* __restrict__ dones,
    uint8_t* __restrict__ fb_ply, int32_t* __restrict__ plies_out, int32_t* __restrict__ fb_cnt,
    unsigned long long* __restrict__ wdl, unsigned long long* __restrict__ wdl_vs, PlayNtupleTd td, Rng rng,
    uint64_t ctr) {
    constexpr int W = Geo<N>::W, NN = N * N, G = SOLVE_GROUP;
    static_assert(NN <= 256, "a square fits the reduction keys' low byte");
    static_assert(G * 8 == SOLVE_BLOCK, "eight lanes a board form a target");
    __shared__ uint32_t g_plan[2][NTUPLE_PLAN_WORDS];
    __shared__ uint64_t g_M[G][W], g_O[G][W], g_moves[G][W];  // a wanting board's mover, opponent and root moves
    __shared__ int g_cnt[G];    // its tasks; 0: the board wants no search this round
    __shared__ int g_depth[G], g_side[G];
    __shared__ unsigned long long g_key[G];  // max of root_key
    __shared__ int g_gkey[G];                // max of play_search_flip_key: the fallback's move
    __shared__ unsigned int g_over[G];
    __shared__ int g_act[G], g_learn[G], g_tgt[G];  // td: the round's move, whether its row learns, its target
    const int lane = threadIdx.x;
    // the plans first (key.tuples is checked: at most 32), block-uniformly: a plan made for something else
    // changes nothing
    {
        const int wb = NTUPLE_HEAD + NTUPLE_REC * (int)key_b.tuples, ww = NTUPLE_HEAD + NTUPLE_REC * (int)key_w.tuples;
        for (int i = lane; i < wb; i += SOLVE_BLOCK) g_plan[0][i] = side_b.plan[i];
        if (!same)
            for (int i = lane; i < ww; i += SOLVE_BLOCK) g_plan[1][i] = side_w.plan[i];
        __syncthreads();
        if (!ntuple_plan_is(g_plan[0], key_b)) return;
        if (!same && !ntuple_plan_is(g_plan[1], key_w)) return;
    }
    side_b.plan = g_plan[0];
    side_w.plan = same ? g_plan[0] : g_plan[1];
    ctr += *rng.ply_off;  // graph-region offset (oth_graph_end); 0 eagerly
    const long long e0 = (long long)blockIdx.x * G;
    const int ne = (int)(E - e0 < G ? E - e0 : G);
    const bool rows = MODE == PS_PLAY && td.boards != nullptr;  // (a kernel argument: uniform)

    // ---- td: zeros on every row of the block's boards; the rows that learn are stored over them
    if (rows) {
        for (int j = lane; j < n_plies * ne; j += SOLVE_BLOCK) {
            const int p = j / ne, i = j - p * ne;
            const size_t r = (size_t)p * (size_t)E + (size_t)(e0 + i);
#pragma unroll
            for (int k = 0; k < 2 * W; ++k) td.boards[r * 2 * W + k] = 0ull;
            td.meta[r] = 0;
            td.targets[r] = 0;
            td.learn[r] = 0;
        }
    }

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
        g_act[lane] = 0;
        g_learn[lane] = 0;
        g_tgt[lane] = 0;
    }
    __syncthreads();  // (the zeros of the rows are on their way before a row is stored)

    // ---- the rounds
    for (;;) {
        bool want = false;
        if (lane < G) {
            int cnt = 0;
            if (o.owner) {
                // through everything that needs no search: an exploring ply is applied here and the board goes on
                for (;;) {
                    want = o.advance();
                    if (!want) break;
                    const bool sw = MODE == PS_PLAY && (s.meta & M_TURN_WHITE) != 0;
                    const BB<W> mv = s.legal & Geo<N>::BOARD;
                    int k;
                    if (!ntuple_explores(rng.seed, o.id, o.ply_index(), sw ? side_w.explore : side_b.explore,
                                         popcount(mv), k))
                        break;
                    o.apply(select_bit<W>(mv, k), 0);
                }
            }
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
            g_learn[lane] = 0;
        }
        __syncthreads();
        // the tasks: plan, weights, depth and budget are their board's side's.  The count is read from LDS after
        // the barrier: the exit test is block-uniform
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
                const NtupleEval ev{sw ? side_w.plan : side_b.plan, sw ? side_w.weights : side_b.weights,
                                    sw ? side_w.terminal : side_b.terminal};
                return [=](RootTask<N>& s, uint32_t* st) { ntuple_search_step<N>(s, st, max_nodes, depth, ev); };
            },
            [&](const RootTask<N>& s, int i, int a) {
                if (s.over) atomicOr(&g_over[i], 1u);
                else atomicMax(&g_key[i], root_key(s.result, SEARCH_INF, a));
            });
        if (total == 0) break;
        __syncthreads();
        int a = -1;
        bool over = false;
        if (want) {
            over = g_over[lane] != 0u;
            a = over ? 255 - (g_gkey[lane] & 255) : root_key_square(g_key[lane]);
            g_act[lane] = a;
            g_learn[lane] = rows && !over ? 1 : 0;
        }
        if (rows) {
            // the targets: eight lanes a board, lane sym its symmetry's share of H of the next row
            __syncthreads();
            const int i = lane >> 3, sym = lane & 7;
            const bool learn = g_learn[i] != 0;
            const bool sw = g_side[i] != 0;
            const uint32_t* plan = sw ? side_w.plan : side_b.plan;
            const int32_t* wts = sw ? side_w.weights : side_b.weights;
            BB<W> M, O, Mn = zero<W>(), On = zero<W>();
#pragma unroll
            for (int k = 0; k < W; ++k) {
                M.w[k] = g_M[i][k];
                O.w[k] = g_O[i][k];
            }
            const int kind = learn ? ntuple_td_after<N>(M, O, g_act[i], Mn, On) : TD_OVER;
            long long acc = 0;
            if (kind == TD_TURN) acc = ntuple_sum_sym(plan, (int)plan[2], sym, wts, On.w, Mn.w);
            if (kind == TD_PASS) acc = ntuple_sum_sym(plan, (int)plan[2], sym, wts, Mn.w, On.w);
#pragma unroll
            for (int m = 1; m < 8; m <<= 1) acc += __shfl_xor(acc, m);
            if (learn && sym == 0) {
                const int32_t h = kind == TD_OVER ? 0 : ntuple_value((int64_t)acc + (int64_t)wts[plan[4]], (int)plan[3]);
                g_tgt[i] = ntuple_td_value(kind, popcount(Mn) - popcount(On), h);
            }
            __syncthreads();
        }
        if (want) {
            if (rows && !over) {  // the row before the ply, in the exchange format
                const size_t r = (size_t)o.p * (size_t)E + (size_t)o.e;
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    td.boards[r * 2 * W + k] = s.black.w[k];
                    td.boards[r * 2 * W + W + k] = s.white.w[k];
                }
                td.meta[r] = (uint16_t)s.meta;
                td.targets[r] = g_tgt[lane];
                td.learn[r] = 1;
            }
            o.apply(a, over ? 1 : 0);
        }
    }

    // ---- the boards back, the call's outputs, the tallies: two blocks share a W/D/L slot (the handle has one
    // per 16 boards)
    o.finish(boards, meta, legal, plies_out, fb_cnt, wdl, wdl_vs, (size_t)(blockIdx.x >> 1));
}

}  // namespace oth_dev
#endif
