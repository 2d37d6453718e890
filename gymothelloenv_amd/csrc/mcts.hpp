// mcts.hpp -- oth_mcts: a UCT-style tree search per board with random-playout
// leaf evaluation (the spec is the header's comment on oth_mcts: every output
// is an integer function of the board and the parameters).
//
// The tree of a board lives in its slice of the caller's workspace, T nodes of
// MctsTree<N>::WORDS 64-bit words:
//   [0, W)      black's discs            [W, 2W)  white's
//   [2W, 3W)    the node's moves not yet made into children
//   [3W]        v | w << 32
//   [3W + 1]    first child | parent << 32
//   [3W + 2]    k | turn << 32
// k is the node's move count (0: the node is terminated), first child 0: no
// slots reserved yet (slot 0 is the root, never a child).  A node keeps its
// parent's index, so the path of an iteration needs no array: the backup walks
// the parent links.  Every index is a whole 32-bit half of its word: with the
// indices packed as 24-bit fields beside k and the turn, the compiler dropped
// the field's mask in front of the node address's 64-bit multiply-add
// (v_mad_u64_u32 on the unmasked dword), and the kernel read far outside the
// workspace.
//
// The part outside __HIPCC__ is plain host/device code over bitboard.hpp and
// root_tasks.hpp's fill-free solve_flips / solve_legal: isqrt, the key, the
// descent (reserve, make-child, select), the backup, the outputs, and a
// one-board driver mcts_host whose playouts use the generic rules
// (tests/host/mcts_host.cpp compiles it with g++).
//
// Device mapping (k_mcts).  A block is one wave and
// serves G = 64 / R consecutive boards: lane l belongs to board l / R and plays
// playout l % R of every evaluated node; lanes beyond G R idle.  Every node
// field is read and written by the board's first lane (its leader) alone: a
// node written by one lane is not safely visible to another lane of the wave
// without a fence.  The other lanes get the leaf's position by __shfl from the
// leader, and the leader gets the playouts' outcome counts from ballots masked
// to the board's lane segment.  A tree is owned by one wave: no atomics.
#pragma once
#include <math.h>

#include "root_tasks.hpp"

namespace oth {

constexpr int MCTS_MAX_ITERATIONS = 65535, MCTS_MAX_PLAYOUTS = 64, MCTS_MAX_C = 65535;
constexpr int MCTS_MAX_TREE_NODES = 1 << 24;
constexpr int MCTS_DONE = 0, MCTS_TERMINATED = 1, MCTS_NO_MOVE = 3;
constexpr int MCTS_MAX_PLIES = 256;  // > N*N - 4 + 1: every playout ply places a disc

struct MctsParams {
    int I, R, C;
    uint32_t T;
    uint64_t seed;
    uint64_t g0;  // the counter of playout ply 0: counter * 256
    uint32_t id_key;
};

// the exact floor square root of x <= 2^32: the double's root (x is exact in a
// double, the root correctly rounded), then an integer correction
OTH_HD uint32_t mcts_isqrt(uint64_t x) {
    uint64_t s = (uint64_t)sqrt((double)x);
    while (s * s > x) --s;
    while ((s + 1) * (s + 1) <= x) ++s;
    return (uint32_t)s;
}

// floor(2^15 w_c / (v_c R)) + floor(cs / (1 + v_c)), cs = C isqrt(2^16 v_p) < 2^32.
// The first quotient is below 2^17 (w_c <= 2 v_c R) and both operands are exact
// in a double, so the double's quotient is within one of it: an integer
// correction makes it exact without a 64-bit division.
OTH_HD uint64_t mcts_key(uint32_t w_c, uint32_t v_c, uint32_t cs, int R) {
    const uint64_t num = (uint64_t)w_c << 15, den = (uint64_t)v_c * (uint64_t)R;
    uint64_t q = (uint64_t)((double)num / (double)den);
    if (q * den > num) --q;
    else if ((q + 1) * den <= num) ++q;
    return q + (uint64_t)(cs / (1u + v_c));
}

template <int N>
struct MctsTree {
    static constexpr int W = Geo<N>::W, NN = N * N;
    static constexpr int WORDS = 3 * W + 3;
    static constexpr int AT_VW = 3 * W, AT_LINK = 3 * W + 1, AT_INFO = 3 * W + 2;

    uint64_t* t;  // the board's T nodes
    uint32_t used;

    OTH_HD uint64_t* node(uint32_t i) const { return t + (size_t)i * WORDS; }

    // a new node: a position as oth_step with flags 0 leaves it (tw: white is to move; moves: the
    // side to move's, none: terminated), v = w = 0, no reservation
    OTH_HD void put(uint32_t i, const BB<W>& black, const BB<W>& white, bool tw, const BB<W>& moves,
                    uint32_t parent) const {
        uint64_t* nd = node(i);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            nd[j] = black.w[j];
            nd[W + j] = white.w[j];
            nd[2 * W + j] = moves.w[j];
        }
        nd[AT_VW] = 0ull;
        nd[AT_LINK] = (uint64_t)parent << 32;
        nd[AT_INFO] = (uint64_t)(uint32_t)popcount(moves) | (uint64_t)tw << 32;
    }

    // One iteration's descent from the root (the header's step 1): the node to evaluate.
    OTH_HD uint32_t descend(uint32_t T, int R, int C) {
        uint32_t cur = 0;
        for (int level = 0; level < NN; ++level) {  // (a path places a disc per level: never NN levels)
            uint64_t* nd = node(cur);
            const uint64_t link = nd[AT_LINK], info = nd[AT_INFO];
            const uint32_t k = (uint32_t)info;
            if (k == 0) break;  // terminated
            uint32_t first = (uint32_t)link;
            if (first == 0) {  // no reservation yet
                if (used + k > T) break;  // the tree is full: cur stays a leaf
                first = used;
                used += k;
                nd[AT_LINK] = link | (uint64_t)first;
            }
            BB<W> rem;
#pragma unroll
            for (int j = 0; j < W; ++j) rem.w[j] = nd[2 * W + j];
            if (any(rem)) {  // the next child: the lowest square not yet made, oth_step's ply with flags 0
                const int a = lowest_square<W>(rem);
                const BB<W> bit = square<W>(a);
                const uint32_t slot = first + (k - (uint32_t)popcount(rem));
                BB<W> B, Wt;
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    nd[2 * W + j] = rem.w[j] & ~bit.w[j];
                    B.w[j] = nd[j];
                    Wt.w[j] = nd[W + j];
                }
                const bool tw = (info >> 32) != 0;
                const BB<W> M = pick(tw, Wt, B), O = pick(tw, B, Wt);
                const BB<W> fl = solve_flips<N>(M, O, a);
                const BB<W> Mn = M | fl | bit, On = O & ~fl;
                BB<W> L = solve_legal<N>(On, Mn);
                const bool pass = !any(L);  // the reply is a pass: the same colour moves again, or the game is over
                if (pass) L = solve_legal<N>(Mn, On);
                put(slot, pick(tw, On, Mn), pick(tw, Mn, On), pass ? tw : !tw, L, cur);
                cur = slot;
                break;
            }
            // every child is made: the largest key, the lowest square (the lowest slot) of equal keys
            const uint32_t cs = (uint32_t)C * mcts_isqrt((uint64_t)(uint32_t)nd[AT_VW] << 16);
            uint64_t bk = 0;
            uint32_t bi = first;
            for (uint32_t j = 0; j < k; ++j) {
                const uint64_t vw = node(first + j)[AT_VW];
                const uint64_t key = mcts_key((uint32_t)(vw >> 32), (uint32_t)vw, cs, R);
                if (j == 0 || key > bk) {
                    bk = key;
                    bi = first + j;
                }
            }
            cur = bi;
        }
        return cur;
    }

    // the position of node i
    OTH_HD void position(uint32_t i, BB<W>& black, BB<W>& white, bool& tw, bool& term) const {
        const uint64_t* nd = node(i);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            black.w[j] = nd[j];
            white.w[j] = nd[W + j];
        }
        const uint64_t info = nd[AT_INFO];
        tw = (info >> 32) != 0;
        term = (uint32_t)info == 0;
    }

    // The backup of R playouts from cur, n_white won by white and n_draw drawn: v += 1 on the
    // whole path; w += 2 won + drawn for the colour that moved into the node (its parent's side
    // to move) on every node but the root.
    OTH_HD void backup(uint32_t cur, int n_white, int n_draw, int R) const {
        const uint32_t for_white = (uint32_t)(2 * n_white + n_draw);
        const uint32_t for_black = (uint32_t)(2 * (R - n_white - n_draw) + n_draw);
        while (cur != 0) {
            uint64_t* nd = node(cur);
            const uint32_t parent = (uint32_t)(nd[AT_LINK] >> 32);
            const bool ptw = (node(parent)[AT_INFO] >> 32) != 0;
            nd[AT_VW] += 1ull + ((uint64_t)(ptw ? for_white : for_black) << 32);
            cur = parent;
        }
        node(0)[AT_VW] += 1ull;
    }

    // The outputs of a searched board.  moves: the root's move list (the stored possible_moves).
    OTH_HD void outputs(const BB<W>& moves, int32_t* visits, int32_t* wins2, int32_t* best) const {
        const uint64_t* root = node(0);
        const uint32_t first = (uint32_t)root[AT_LINK];
        BB<W> rem;
#pragma unroll
        for (int j = 0; j < W; ++j) rem.w[j] = root[2 * W + j];
        const BB<W> made = moves & ~rem;
        uint32_t slot = first, bv = 0, bw = 0;
        int ba = -1;
        for (int a = 0; a < NN; ++a) {
            uint32_t v = 0, w = 0;
            if (test(made, a)) {
                const uint64_t vw = node(slot++)[AT_VW];
                v = (uint32_t)vw;
                w = (uint32_t)(vw >> 32);
                if (ba < 0 || v > bv || (v == bv && w > bw)) {
                    ba = a;
                    bv = v;
                    bw = w;
                }
            }
            visits[a] = (int32_t)v;
            if (wins2) wins2[a] = (int32_t)w;
        }
        if (best) *best = ba;
    }
};

// what a board gets without a search
template <int N>
OTH_HD int mcts_status(const BB<Geo<N>::W>& stored, uint32_t meta) {
    if (meta & 2u) return MCTS_TERMINATED;
    if (!any(stored & Geo<N>::BOARD)) return MCTS_NO_MOVE;
    return MCTS_DONE;
}

// One playout with the generic rules (the host driver's): uniformly random legal moves to the
// end from (black, white), tw to move, as oth_playouts' ROOT mode plays them.  Returns the
// winner's colour, +1 white / 0 / -1 black.
template <int N>
inline int mcts_playout_host(BB<Geo<N>::W> black, BB<Geo<N>::W> white, bool tw, uint64_t seed, uint32_t id,
                             uint64_t g0) {
    constexpr int W = Geo<N>::W;
    BB<W> M = tw ? white : black, O = tw ? black : white;
    BB<W> L = legal_moves<N>(M, O);
    for (int p = 0; p < MCTS_MAX_PLIES && any(L); ++p) {
        const uint32_t u = action_draw(seed, id, g0 + (uint64_t)p);
        const int a = select_bit(L, scale_index(u, popcount(L)));
        const BB<W> bit = square<W>(a);
        const BB<W> fl = flips<N>(M, O, bit);
        const BB<W> Mn = M | fl | bit, On = O & ~fl;
        L = legal_moves<N>(On, Mn);
        if (any(L)) {
            M = On;
            O = Mn;
            tw = !tw;
        } else {  // a pass, or the end
            L = legal_moves<N>(Mn, On);
            M = Mn;
            O = On;
        }
    }
    const int d = tw ? popcount(M) - popcount(O) : popcount(O) - popcount(M);  // white - black
    return d > 0 ? 1 : (d < 0 ? -1 : 0);
}

// One board on the host: the whole algorithm.  tree: T * MctsTree<N>::WORDS words, uninitialised.
// visits / wins2: N*N entries.  Returns the status.
template <int N>
inline int mcts_host(const uint64_t* black, const uint64_t* white, const uint64_t* stored, uint32_t meta,
                     uint32_t env_id, const MctsParams& p, uint64_t* tree, int32_t* visits, int32_t* wins2,
                     int32_t* best, int32_t* tree_nodes) {
    constexpr int W = Geo<N>::W, NN = N * N;
    BB<W> B, Wt, Lg;
    for (int i = 0; i < W; ++i) {
        B.w[i] = black[i];
        Wt.w[i] = white[i];
        Lg.w[i] = stored[i];
    }
    const int st = mcts_status<N>(Lg, meta);
    if (st != MCTS_DONE) {
        for (int a = 0; a < NN; ++a) visits[a] = wins2[a] = 0;
        *best = -1;
        *tree_nodes = 1;
        return st;
    }
    const BB<W> moves = Lg & Geo<N>::BOARD;
    MctsTree<N> tr{tree, 1u};
    tr.put(0, B, Wt, (meta & 1u) != 0, moves, 0);
    for (int i = 0; i < p.I; ++i) {
        const uint32_t cur = tr.descend(p.T, p.R, p.C);
        BB<W> cb, cw;
        bool tw, term;
        tr.position(cur, cb, cw, tw, term);
        int n_white = 0, n_draw = 0;
        for (int r = 0; r < p.R; ++r) {
            const uint32_t id = p.id_key + (env_id * (uint32_t)p.I + (uint32_t)i) * (uint32_t)p.R + (uint32_t)r;
            const int win = mcts_playout_host<N>(cb, cw, tw, p.seed, id, p.g0);  // (a terminated node: no ply)
            n_white += win > 0;
            n_draw += win == 0;
        }
        tr.backup(cur, n_white, n_draw, p.R);
    }
    tr.outputs(moves, visits, wins2, best);
    *tree_nodes = (int32_t)tr.used;
    return MCTS_DONE;
}

}  // namespace oth

#if defined(__HIPCC__)
#include "playouts.hpp"

namespace oth_dev {

static_assert(MCTS_MAX_ITERATIONS == OTH_MCTS_MAX_ITERATIONS && MCTS_MAX_PLAYOUTS == OTH_MCTS_MAX_PLAYOUTS &&
                  MCTS_MAX_C == OTH_MCTS_MAX_C && MCTS_MAX_TREE_NODES == OTH_MCTS_MAX_TREE_NODES,
              "the header's limits");
static_assert(MCTS_DONE == OTH_MCTS_DONE && MCTS_TERMINATED == OTH_MCTS_TERMINATED &&
                  MCTS_NO_MOVE == OTH_MCTS_NO_MOVE,
              "the header's status codes");
static_assert(MCTS_MAX_PLIES == PLAYOUT_MAX_PLIES, "oth_playouts' bound");

constexpr int MCTS_BLOCK = 64;  // one wave a block

__device__ __forceinline__ uint64_t shfl64(uint64_t x, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, src, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), src, 64);
    return (uint64_t)hi << 32 | lo;
}

template <int N>
__global__ __launch_bounds__(MCTS_BLOCK) void k_mcts(const uint64_t* __restrict__ boards,
                                                     const uint16_t* __restrict__ meta,
                                                     const uint64_t* __restrict__ legal, int E, MctsParams p,
                                                     uint32_t id_base, uint64_t* __restrict__ ws,
                                                     int32_t* __restrict__ visits, int32_t* __restrict__ wins2,
                                                     int32_t* __restrict__ best, int32_t* __restrict__ tree_nodes,
                                                     uint8_t* __restrict__ status) {
    using Eng = PlayoutEng<N>;
    using Tree = MctsTree<N>;
    constexpr int W = Geo<N>::W, NN = N * N;
    __shared__ __attribute__((aligned(16))) uint64_t lds_rays[Eng::RAY_WORDS > 0 ? Eng::RAY_WORDS : 1];
    __shared__ __attribute__((aligned(16))) uint64_t lds_sel[256];
    const uint8_t* sel8 = reinterpret_cast<const uint8_t*>(lds_sel);
    const int lane = threadIdx.x;
    if constexpr (W <= 2) {
        for (int i = lane; i < 256; i += MCTS_BLOCK) lds_sel[i] = sel8_word((uint32_t)i);
        if constexpr (W == 2) {  // FillsW::fill's table, by one wave
            BB<W>* r = reinterpret_cast<BB<W>*>(lds_rays);
            for (int i = lane; i < 8 * NN; i += MCTS_BLOCK) r[i] = ray_from<N>(i / NN, i % NN);
        }
        __syncthreads();
    }
    const int R = p.R, G = MCTS_BLOCK / R;
    const int gi = lane / R, r = lane - gi * R;
    const long long e = (long long)blockIdx.x * G + gi;
    const bool active = gi < G && e < E;
    const bool leader = active && r == 0;
    const int src = (gi < G ? gi : G - 1) * R;  // the board's leader lane (an idle lane reads a lane that exists)
    const unsigned long long seg = (R == 64 ? ~0ull : (1ull << R) - 1ull) << (src & 63);

    // the leader classifies the board, writes the outputs of one that is not searched, and the root
    Tree tr{ws, 1u};
    BB<W> moves = zero<W>();
    bool searched = false;
    if (leader) {
        tr.t = ws + (size_t)e * p.T * Tree::WORDS;
        BB<W> B, Wt, Lg;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            B.w[i] = boards[(size_t)e * 2 * W + i];
            Wt.w[i] = boards[(size_t)e * 2 * W + W + i];
            Lg.w[i] = legal[(size_t)e * W + i];
        }
        const uint32_t m = meta[e];
        const int st = mcts_status<N>(Lg, m);
        if (status) status[e] = (uint8_t)st;
        if (st == MCTS_DONE) {
            searched = true;
            moves = Lg & Geo<N>::BOARD;
            tr.put(0, B, Wt, (m & M_TURN_WHITE) != 0, moves, 0);
        } else {
            for (int a = 0; a < NN; ++a) {
                visits[(size_t)e * NN + a] = 0;
                if (wins2) wins2[(size_t)e * NN + a] = 0;
            }
            if (best) best[e] = -1;
            if (tree_nodes) tree_nodes[e] = 1;
        }
    }
    if (!__any(searched)) return;
    const bool plays = active && __shfl((int)searched, src, 64) != 0;
    const Eng eng(0, lds_rays);
    const uint32_t id0 = p.id_key + (id_base + (uint32_t)e) * (uint32_t)p.I * (uint32_t)R + (uint32_t)r;

    for (int it = 0; it < p.I; ++it) {  // wave-uniform
        uint32_t cur = 0;
        BB<W> cb = zero<W>(), cw = zero<W>();
        bool ctw = false, cterm = true;
        if (searched) {
            cur = tr.descend(p.T, R, p.C);
            tr.position(cur, cb, cw, ctw, cterm);
        }
        // the leaf's position to the board's lanes
        Lane<N> s;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            s.black.w[i] = shfl64(cb.w[i], src);
            s.white.w[i] = shfl64(cw.w[i], src);
        }
        const int flags = __shfl((int)ctw | (int)cterm << 1, src, 64);
        bool tw = (flags & 1) != 0;
        bool live = plays && !(flags & 2);
        const uint32_t id = id0 + (uint32_t)it * (uint32_t)R;
        int outcome;  // the winner's colour
        // The playout: oth_playouts' ROOT-mode ply loop (playouts.hpp k_playouts), duplicated here
        // and not shared through a function, so that k_playouts' measured code stays as it is:
        // one-word boards as (mover, opponent) words with the Fills engine, the others through step_lane.
        if constexpr (W == 1) {
            uint64_t M = tw ? s.white.w[0] : s.black.w[0], O = tw ? s.black.w[0] : s.white.w[0];
            BB<1> mb, ob;
            mb.w[0] = M;
            ob.w[0] = O;
            uint64_t L = eng.legal(mb, ob).w[0];  // the mover's moves, and the engine's fills of this position
            live = live && L != 0;
            auto fast = [&](uint32_t u) __attribute__((always_inline)) {
                if (live) {
                    const int pa = select64_tab(L, scale_index(u, popc64(L)), sel8);
                    BB<1> dummy;
                    dummy.w[0] = 0;
                    const uint64_t fl = eng.flip(dummy, dummy, pa).w[0];
                    const uint64_t mv = 1ull << pa;
                    BB<1> pb, nb;
                    pb.w[0] = O & ~fl;  // the next mover
                    nb.w[0] = M | fl | mv;
                    uint64_t Ln = eng.legal(pb, nb).w[0];
                    const bool pass = Ln == 0;
                    if (pass) Ln = eng.legal(nb, pb).w[0];  // the mover moves again (fills recomputed)
                    M = pass ? nb.w[0] : pb.w[0];
                    O = pass ? pb.w[0] : nb.w[0];
                    L = Ln;
                    tw ^= !pass;
                    live = Ln != 0;
                }
            };
            for (int q = 0; q < MCTS_MAX_PLIES && __any(live); q += 4) {
                const U4 d4 = philox4(p.seed, id, (p.g0 >> 2) + (uint64_t)(q >> 2), RNG_ACTION);
                fast(d4.x);
                fast(d4.y);
                fast(d4.z);
                fast(d4.w);
            }
            outcome = sign_i32(tw ? popc64(M) - popc64(O) : popc64(O) - popc64(M));  // WHITE_DISK = +1
        } else {
            s.meta = tw ? M_TURN_WHITE : 0u;
            {
                BB<W> P, O;  // word-wise selects, as FillsW::prime
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    P.w[i] = tw ? s.white.w[i] : s.black.w[i];
                    O.w[i] = tw ? s.black.w[i] : s.white.w[i];
                }
                s.legal = eng.legal(P, O);
            }
            live = live && any(s.legal);
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
                    if (dd) live = false;
                }
            };
            for (int q = 0; q < MCTS_MAX_PLIES && __any(live); q += 4) {
                const U4 d4 = philox4(p.seed, id, (p.g0 >> 2) + (uint64_t)(q >> 2), RNG_ACTION);
                ply(d4.x);
                ply(d4.y);
                ply(d4.z);
                ply(d4.w);
            }
            outcome = sign_i32(popcount(s.white) - popcount(s.black));  // the final board's count (flags 0)
        }
        // the board's outcome counts: ballots masked to its lane segment
        const unsigned long long bw = __ballot(plays && outcome > 0), bd = __ballot(plays && outcome == 0);
        if (searched) tr.backup(cur, __popcll(bw & seg), __popcll(bd & seg), R);
    }
    if (searched) {
        tr.outputs(moves, visits + (size_t)e * NN, wins2 ? wins2 + (size_t)e * NN : nullptr, best ? best + e : nullptr);
        if (tree_nodes) tree_nodes[e] = (int32_t)tr.used;
    }
}

}  // namespace oth_dev
#endif
