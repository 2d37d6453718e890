// puct.hpp -- oth_puct_begin / _advance / _result: a tree search per board whose
// leaves are evaluated outside the library (a policy and value network between
// launches), one simulation per launch for all boards (the spec is the header's
// comment on oth_puct_begin: every output is an integer function of the board,
// the parameters and the integers supplied); and oth_puct_pick / oth_puct_reroot,
// self-play on that tree: the move of a search, and the search carried to the
// position the handle has reached, the played child's subtree compacted in
// place (the header's comment on oth_puct_pick).
//
// The workspace, in 64-bit words (PuctWs; E boards, T nodes a board):
//   [0]                   the tag of the search that began here (puct_tag)
//   [1]                   unused (keeps what follows 16-byte aligned in itself)
//   [2, 2 + 2E)           a board's header: used | pending leaf << 32, then
//                         kind | status << 8 | (the handle's meta at begin) << 32
//   then [E][2W], [E][W]  the pending leaves' boards and moves, exchange format:
//   and ceil(E / 4)       their meta (uint16 [E]); the observation kernels read these
//   then E T WORDS        the trees
// A node is PuctTree<N>::WORDS words:
//   [0, W)      black's discs            [W, 2W)  white's
//   [2W, 3W)    the node's moves (the side to move's; none: terminated)
//   [3W]        w, an int64
//   [3W + 1]    v | P << 32
//   [3W + 2]    first child | parent << 32
//   [3W + 3]    k | (turn | made << 1 | terminated << 2 | square << 8) << 32
// first child 0: no children reserved (slot 0 is the root, never a child).  A
// child exists from its parent's expansion on (square, P, v = w = 0, its parent);
// its position words are written when a selection first moves to it (made).
// Every node index is a whole 32-bit half of its word, as mcts.hpp's (its
// header comment has the reason).  A node keeps its parent's index: the backup
// walks the links and the path needs no array.
//
// A batch search (oth_puct_begin_batch / _advance_batch / _reroot_batch: K leaves a
// board per launch under virtual loss, the header's comment on
// oth_puct_begin_batch) keeps that layout unchanged, a board's header kind NONE
// throughout, and adds an extension behind it (PuctBatchWs), from the next even word:
//   [0], [1]              the tags of the batch search: ~puct_tag, puct_batch_tag(K)
//   then [EK][2W], [EK][W] and ceil(EK / 4): the leaf arrays of the E K rows, as above
//   then [E][K]           a board's slots: node | kind << 32
// The paths of a launch's earlier slots are counted in bits 24 .. 31 of a node's v
// half (v < 2^24, K <= 64) while one board's selection runs, and are taken out
// again before the call returns: between launches every word is what the plain
// calls leave, which is why result, pick, compact and the wave sweep read it as it is.
//
// The part outside __HIPCC__ is plain host/device code over bitboard.hpp and
// root_tasks.hpp's fill-free solve_flips / solve_legal: the layout, the key, one
// board's begin / apply / select / leaf / outputs, and the three calls for one
// board (puct_begin_board, puct_advance_board, puct_result_board), which
// tests/host/puct_host.cpp compiles with g++ and loops over the boards; then
// puct_pick_board and puct_reroot_board (classify, sweep, finish), which
// tests/host/puct_play_host.cpp compiles the same way; and the batch calls for one
// board (puct_begin_batch_board, puct_advance_batch_board, puct_reroot_finish_batch),
// which tests/host/puct_batch_host.cpp compiles.
//
// Device mapping: one lane per board runs those
// functions.  Every word of a board's tree, header and leaf is read and written
// by that one lane, so there is nothing to fence and no atomic; launches on a
// stream order one simulation after another.  The observation of the leaves is
// a second launch of the observation kernels on the workspace's leaf arrays.
// The one exception is the re-root's compaction, k_puct_reroot_sweep: a wave
// per board between two lane-per-board launches (its comment has the ordering).
#pragma once
#include <math.h>

#include "mcts.hpp"

#ifndef OTH_PUCT_SELECT_CHUNK
// children whose words the selection loads ahead of their keys (1: a load per key)
#define OTH_PUCT_SELECT_CHUNK 4
#endif
#ifndef OTH_PUCT_REROOT_LANE
// 1: oth_puct_reroot as one launch, a lane per board (k_puct_reroot_lane); 0, the shipped mapping: the
// compaction on a wave per board between two lane-per-board launches (DESIGN.md sections 4 and 5)
#define OTH_PUCT_REROOT_LANE 0
#endif
#ifndef OTH_PUCT_REROOT_LDS
// the wave sweep's forwarding table in LDS, in slots (4 bytes each); a longer subtree goes in place on one lane
#define OTH_PUCT_REROOT_LDS 4096
#endif

namespace oth {

constexpr int PUCT_VALUE_ONE = 32768, PUCT_PRIOR_MAX = 65535, PUCT_MAX_C = 65535;
constexpr int PUCT_MAX_TREE_NODES = 1 << 24, PUCT_MAX_SIMS = (1 << 24) - 1;
constexpr int PUCT_LEAF_NONE = 0, PUCT_LEAF_EXPAND = 1, PUCT_LEAF_VALUE = 2, PUCT_LEAF_TERMINAL = 3;
constexpr int PUCT_MAX_LEAVES = 64;       // slots a board in a batch call
constexpr int PUCT_REROOT_KEPT = 0xff;    // a header's kind between the steps of one oth_puct_reroot: the board is kept
constexpr uint32_t PUCT_RNG_PICK = 4u;    // Philox purpose word of oth_puct_pick's draw (state.hpp RNG_PUCT_PICK)

// floor(num / den) for num < 2^53, 0 < den < 2^53: both are exact in a double, the
// double's quotient is within one of it, and an integer correction makes it
// exact without a 64-bit division (mcts_key's way)
OTH_HD uint64_t puct_floor_div(uint64_t num, uint64_t den) {
    uint64_t q = (uint64_t)((double)num / (double)den);
    if (q * den > num) --q;
    else if ((q + 1) * den <= num) ++q;
    return q;
}

// floor(w / v) toward minus infinity, |w| <= 2^15 v, 0 < v < 2^24
OTH_HD int64_t puct_floor_q(int64_t w, uint32_t v) {
    const uint64_t a = (uint64_t)(w < 0 ? -w : w);
    const uint64_t q = puct_floor_div(a, (uint64_t)v);
    if (w >= 0) return (int64_t)q;
    return q * (uint64_t)v == a ? -(int64_t)q : -(int64_t)q - 1;
}

// cs = C isqrt(2^16 v_p) < 2^36; the key is q_c + floor(cs P_c / (2^17 (1 + v_c))), its numerator below 2^52
OTH_HD int64_t puct_key(int64_t w_c, uint32_t v_c, uint32_t P_c, uint64_t cs) {
    const int64_t q = v_c == 0 ? 0 : puct_floor_q(w_c, v_c);
    return q + (int64_t)puct_floor_div(cs * (uint64_t)P_c, (uint64_t)(1u + v_c) << 17);
}

// the words of one node, of the workspace, and the tag of a search (n, E, T: what an advance must match)
constexpr int puct_node_words(int n) { return 3 * ((n * n + 63) / 64) + 4; }
constexpr uint64_t puct_ws_words(int n, uint64_t E, uint64_t T) {
    return 2u + 2u * E + 3u * (uint64_t)((n * n + 63) / 64) * E + (E + 3u) / 4u + E * T * (uint64_t)puct_node_words(n);
}
OTH_HD uint64_t puct_tag(int n, uint32_t E, uint32_t T) {
    return 0x7075637400000000ull ^ ((uint64_t)(uint32_t)n << 56) ^ ((uint64_t)T << 32) ^ (uint64_t)E;
}

// a batch search's workspace: the plain one, then from the next even word the extension
constexpr uint64_t puct_batch_ext_word(int n, uint64_t E, uint64_t T) { return (puct_ws_words(n, E, T) + 1u) & ~1ull; }
constexpr uint64_t puct_batch_ws_words(int n, uint64_t E, uint64_t T, uint64_t K) {
    return puct_batch_ext_word(n, E, T) + 2u + 3u * (uint64_t)((n * n + 63) / 64) * E * K + (E * K + 3u) / 4u + E * K;
}
OTH_HD uint64_t puct_batch_tag(uint32_t K) { return 0x7075637462617400ull | (uint64_t)K; }

template <int N>
struct PuctWs {
    static constexpr int W = Geo<N>::W;
    uint64_t* base;
    uint32_t E, T;
    OTH_HD uint64_t* tag() const { return base; }
    OTH_HD uint64_t* hdr(uint32_t e) const { return base + 2 + 2 * (size_t)e; }
    OTH_HD uint64_t* leaf_boards() const { return base + 2 + 2 * (size_t)E; }
    OTH_HD uint64_t* leaf_legal() const { return leaf_boards() + 2 * W * (size_t)E; }
    OTH_HD uint16_t* leaf_meta() const { return reinterpret_cast<uint16_t*>(leaf_legal() + W * (size_t)E); }
    OTH_HD uint64_t* tree(uint32_t e) const {
        return leaf_legal() + W * (size_t)E + ((size_t)E + 3) / 4 + (size_t)e * T * (size_t)puct_node_words(N);
    }
};

// the extension of a batch search behind PuctWs: R = E K rows of leaves (the accessors' names are
// PuctWs' own, so that puct_write_leaf serves both)
template <int N>
struct PuctBatchWs {
    static constexpr int W = Geo<N>::W;
    PuctWs<N> plain;
    uint32_t K;
    OTH_HD size_t rows() const { return (size_t)plain.E * K; }
    OTH_HD uint64_t* ext() const { return plain.base + puct_batch_ext_word(N, plain.E, plain.T); }
    OTH_HD uint64_t* leaf_boards() const { return ext() + 2; }
    OTH_HD uint64_t* leaf_legal() const { return leaf_boards() + 2 * W * rows(); }
    OTH_HD uint16_t* leaf_meta() const { return reinterpret_cast<uint16_t*>(leaf_legal() + W * rows()); }
    OTH_HD uint64_t* slots(uint32_t e) const { return leaf_legal() + W * rows() + (rows() + 3) / 4 + (size_t)e * K; }
    OTH_HD void put_tags() const {
        *plain.tag() = puct_tag(N, plain.E, plain.T);
        ext()[0] = ~puct_tag(N, plain.E, plain.T);
        ext()[1] = puct_batch_tag(K);
    }
    // a begin_batch of this geometry, T and K wrote the workspace
    OTH_HD bool begun() const {
        return *plain.tag() == puct_tag(N, plain.E, plain.T) && ext()[0] == ~puct_tag(N, plain.E, plain.T) &&
               ext()[1] == puct_batch_tag(K);
    }
};

// the caller's leaf arrays of one call (oth_puct_leaves without the observation), each may be null
struct PuctLeaves {
    uint8_t* kind;
    uint64_t* boards;
    uint16_t* meta;
    uint64_t* legal;
};

template <int N>
struct PuctTree {
    static constexpr int W = Geo<N>::W, NN = N * N;
    static constexpr int WORDS = 3 * W + 4;
    static constexpr int AT_W = 3 * W, AT_VP = 3 * W + 1, AT_LINK = 3 * W + 2, AT_INFO = 3 * W + 3;
    static constexpr uint32_t F_TURN = 1u, F_MADE = 2u, F_TERM = 4u;
    static constexpr uint32_t F_KEEP = 8u, F_HEAD = 16u;  // compact()'s marks: set during a re-root's sweep only

    uint64_t* t;  // the board's T nodes
    uint32_t used;

    OTH_HD uint64_t* node(uint32_t i) const { return t + (size_t)i * WORDS; }

    // the position of a made node: a position as oth_step with flags 0 leaves it (tw: white is to
    // move; moves: the side to move's, none: terminated)
    OTH_HD void put_position(uint32_t i, const BB<W>& black, const BB<W>& white, bool tw, const BB<W>& moves,
                             uint32_t sq) const {
        uint64_t* nd = node(i);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            nd[j] = black.w[j];
            nd[W + j] = white.w[j];
            nd[2 * W + j] = moves.w[j];
        }
        const uint32_t k = (uint32_t)popcount(moves);
        nd[AT_INFO] = (uint64_t)k | (uint64_t)((tw ? F_TURN : 0u) | F_MADE | (k == 0 ? F_TERM : 0u) | sq << 8) << 32;
    }

    OTH_HD void put_root(const BB<W>& black, const BB<W>& white, bool tw, const BB<W>& moves) {
        put_position(0, black, white, tw, moves, 0u);
        uint64_t* nd = node(0);
        nd[AT_W] = 0ull;
        nd[AT_VP] = 0ull;
        nd[AT_LINK] = 0ull;
        used = 1u;
    }

    OTH_HD void position(uint32_t i, BB<W>& black, BB<W>& white, BB<W>& moves) const {
        const uint64_t* nd = node(i);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            black.w[j] = nd[j];
            white.w[j] = nd[W + j];
            moves.w[j] = nd[2 * W + j];
        }
    }
    OTH_HD uint32_t flags(uint32_t i) const { return (uint32_t)(node(i)[AT_INFO] >> 32); }

    // the kind of a leaf without reserved children (the header's selection rule)
    OTH_HD int leaf_kind(uint32_t i, uint32_t T) const {
        const uint64_t info = node(i)[AT_INFO];
        if ((uint32_t)(info >> 32) & F_TERM) return PUCT_LEAF_TERMINAL;
        return (uint64_t)used + (uint32_t)info <= (uint64_t)T ? PUCT_LEAF_EXPAND : PUCT_LEAF_VALUE;
    }

    // Steps 1 to 3 of an advance: the value of leaf L for its side to move, its expansion, the backup.
    // priors: the board's N*N, read at the leaf's moves only.
    OTH_HD void apply(uint32_t L, int kind, uint32_t T, const int32_t* priors, int32_t value) {
        uint64_t* nd = node(L);
        BB<W> B, Wt, moves;
        position(L, B, Wt, moves);
        const bool s = (flags(L) & F_TURN) != 0;
        int64_t val;
        if (kind == PUCT_LEAF_TERMINAL) {
            const int d = popcount(B) - popcount(Wt);  // black - white
            val = (int64_t)PUCT_VALUE_ONE * sign_i32(s ? -d : d);
        } else {
            val = value < -PUCT_VALUE_ONE ? -PUCT_VALUE_ONE : (value > PUCT_VALUE_ONE ? PUCT_VALUE_ONE : value);
        }
        const uint32_t k = (uint32_t)nd[AT_INFO];
        if (kind == PUCT_LEAF_EXPAND && (uint32_t)nd[AT_LINK] == 0u && (uint64_t)used + k <= (uint64_t)T) {
            const uint32_t first = used;
            used += k;
            nd[AT_LINK] |= (uint64_t)first;
            BB<W> rem = moves;
            for (uint32_t j = 0; j < k; ++j) {  // ascending squares
                const int a = lowest_square<W>(rem);
                rem = rem & ~square<W>(a);
                const int32_t pr = priors[a];
                const uint32_t P = (uint32_t)(pr < 0 ? 0 : (pr > PUCT_PRIOR_MAX ? PUCT_PRIOR_MAX : pr));
                uint64_t* ch = node(first + j);
                ch[AT_W] = 0ull;
                ch[AT_VP] = (uint64_t)P << 32;
                ch[AT_LINK] = (uint64_t)L << 32;
                ch[AT_INFO] = (uint64_t)((uint32_t)a << 8) << 32;
            }
        }
        uint32_t cur = L;
        while (cur != 0) {
            uint64_t* c = node(cur);
            const uint32_t parent = (uint32_t)(c[AT_LINK] >> 32);
            const bool ptw = (flags(parent) & F_TURN) != 0;
            c[AT_W] = (uint64_t)((int64_t)c[AT_W] + (ptw == s ? val : -val));
            c[AT_VP] += 1ull;
            cur = parent;
        }
        node(0)[AT_VP] += 1ull;
    }

    // child c of cur, reserved and not yet made: oth_step's ply with flags 0 on its square, a pass resolved
    OTH_HD void make(uint32_t cur, uint32_t c) const {
        BB<W> B, Wt, mv;
        position(cur, B, Wt, mv);
        const bool tw = (flags(cur) & F_TURN) != 0;
        const uint32_t sq = flags(c) >> 8;
        const int a = (int)sq;
        const BB<W> bit = square<W>(a);
        const BB<W> M = pick(tw, Wt, B), O = pick(tw, B, Wt);
        const BB<W> fl = solve_flips<N>(M, O, a);
        const BB<W> Mn = M | fl | bit, On = O & ~fl;
        BB<W> Lg = solve_legal<N>(On, Mn);
        const bool pass = !any(Lg);  // the reply is a pass: the same colour moves again, or the game is over
        if (pass) Lg = solve_legal<N>(Mn, On);
        put_position(c, pick(tw, On, Mn), pick(tw, Mn, On), pass ? tw : !tw, Lg, sq);
    }

    // Step 4: the descent from the root to the next leaf (made on the way if need be)
    OTH_HD uint32_t select(uint32_t T, int C, int& kind) const {
        uint32_t cur = 0;
        kind = PUCT_LEAF_VALUE;  // (the level bound is never met: a level places a disc)
        for (int level = 0; level < NN + 2; ++level) {
            const uint64_t* nd = node(cur);
            const uint32_t first = (uint32_t)nd[AT_LINK];
            if ((flags(cur) & F_TERM) || first == 0u) {
                kind = leaf_kind(cur, T);
                break;
            }
            const uint32_t k = (uint32_t)nd[AT_INFO];
            const uint64_t cs = (uint64_t)(uint32_t)C * mcts_isqrt((uint64_t)(uint32_t)nd[AT_VP] << 16);
            int64_t bk = 0;
            uint32_t bi = first;
            // ascending squares: the first of equal keys is the lowest.  The children's words are
            // loaded OTH_PUCT_SELECT_CHUNK children at a time ahead of their keys, so a lane waits
            // for memory once per chunk and not once per child (a lane past k re-reads child k - 1).
            for (uint32_t j0 = 0; j0 < k; j0 += OTH_PUCT_SELECT_CHUNK) {
                uint64_t vp[OTH_PUCT_SELECT_CHUNK], cw[OTH_PUCT_SELECT_CHUNK];
#pragma unroll
                for (uint32_t u = 0; u < OTH_PUCT_SELECT_CHUNK; ++u) {
                    const uint64_t* ch = node(first + (j0 + u < k ? j0 + u : k - 1u));
                    vp[u] = ch[AT_VP];
                    cw[u] = ch[AT_W];
                }
#pragma unroll
                for (uint32_t u = 0; u < OTH_PUCT_SELECT_CHUNK; ++u) {
                    const uint32_t j = j0 + u;
                    const int64_t key = puct_key((int64_t)cw[u], (uint32_t)vp[u], (uint32_t)(vp[u] >> 32), cs);
                    if (j < k && (j == 0 || key > bk)) {
                        bk = key;
                        bi = first + j;
                    }
                }
            }
            if (!(flags(bi) & F_MADE)) {
                make(cur, bi);
                cur = bi;
                kind = leaf_kind(cur, T);
                break;
            }
            cur = bi;
        }
        return cur;
    }

    // The selection of one slot of a batch call: select() with every statistic read through the
    // launch's virtual loss, n the paths of earlier slots through a node (bits 24 .. 31 of its v
    // half): v' = v + n, w' = w - PUCT_VALUE_ONE n.  r: the slots reserved so far, this launch's
    // earlier EXPAND leaves included.  kind NONE: the node is already an earlier slot's leaf (no
    // children, not terminated, n > 0), a collision.  With no count set anywhere this is select().
    static constexpr uint32_t V_MASK = 0xffffffu;
    static constexpr int N_SHIFT = 24;
    OTH_HD uint32_t select_vl(uint32_t T, int C, uint32_t& r, int& kind) const {
        uint32_t cur = 0;
        for (int level = 0; level < NN + 2; ++level) {
            const uint64_t* nd = node(cur);
            const uint32_t first = (uint32_t)nd[AT_LINK];
            if ((flags(cur) & F_TERM) || first == 0u) break;
            const uint32_t k = (uint32_t)nd[AT_INFO];
            const uint32_t pv = (uint32_t)nd[AT_VP];
            const uint64_t cs = (uint64_t)(uint32_t)C * mcts_isqrt((uint64_t)((pv & V_MASK) + (pv >> N_SHIFT)) << 16);
            int64_t bk = 0;
            uint32_t bi = first;
            for (uint32_t j0 = 0; j0 < k; j0 += OTH_PUCT_SELECT_CHUNK) {  // (select()'s loads ahead of the keys)
                uint64_t vp[OTH_PUCT_SELECT_CHUNK], cw[OTH_PUCT_SELECT_CHUNK];
#pragma unroll
                for (uint32_t u = 0; u < OTH_PUCT_SELECT_CHUNK; ++u) {
                    const uint64_t* ch = node(first + (j0 + u < k ? j0 + u : k - 1u));
                    vp[u] = ch[AT_VP];
                    cw[u] = ch[AT_W];
                }
#pragma unroll
                for (uint32_t u = 0; u < OTH_PUCT_SELECT_CHUNK; ++u) {
                    const uint32_t j = j0 + u;
                    const uint32_t lo = (uint32_t)vp[u], n = lo >> N_SHIFT;
                    const int64_t key = puct_key((int64_t)cw[u] - (int64_t)PUCT_VALUE_ONE * (int64_t)n, (lo & V_MASK) + n,
                                                 (uint32_t)(vp[u] >> 32), cs);
                    if (j < k && (j == 0 || key > bk)) {
                        bk = key;
                        bi = first + j;
                    }
                }
            }
            if (!(flags(bi) & F_MADE)) {
                make(cur, bi);
                cur = bi;
                break;
            }
            cur = bi;
        }
        const uint64_t info = node(cur)[AT_INFO];
        if ((uint32_t)(info >> 32) & F_TERM) {
            kind = PUCT_LEAF_TERMINAL;
        } else if ((uint32_t)node(cur)[AT_VP] >> N_SHIFT) {
            kind = PUCT_LEAF_NONE;
        } else if ((uint64_t)r + (uint32_t)info <= (uint64_t)T) {
            kind = PUCT_LEAF_EXPAND;
            r += (uint32_t)info;
        } else {
            kind = PUCT_LEAF_VALUE;
        }
        return cur;
    }

    // one path more (d = 1) or less (d = -1) through every node from L up to the root
    OTH_HD void count_path(uint32_t L, int d) const {
        const uint64_t one = 1ull << N_SHIFT;
        for (uint32_t cur = L;; cur = (uint32_t)(node(cur)[AT_LINK] >> 32)) {
            uint64_t* c = node(cur);
            c[AT_VP] = d > 0 ? c[AT_VP] + one : c[AT_VP] - one;
            if (cur == 0u) break;
        }
    }

    // node i as a leaf in exchange format: turn, terminated and winner bits as oth_step sets them
    OTH_HD void leaf(uint32_t i, BB<W>& black, BB<W>& white, BB<W>& moves, uint32_t& meta) const {
        position(i, black, white, moves);
        const uint32_t f = flags(i);
        meta = f & F_TURN;
        if (f & F_TERM) {
            const int d = popcount(white) - popcount(black);
            meta |= 2u | (d > 0 ? 1u : (d < 0 ? 2u : 0u)) << 2;
        }
    }

    // The outputs of a searched board: the root's children by square, the best of them
    OTH_HD void outputs(int32_t* visits, int64_t* value_sums, int32_t* best) const {
        for (int a = 0; a < NN; ++a) {
            visits[a] = 0;
            if (value_sums) value_sums[a] = 0;
        }
        const uint64_t* root = node(0);
        const uint32_t first = (uint32_t)root[AT_LINK], k = first ? (uint32_t)root[AT_INFO] : 0u;
        uint32_t bv = 0;
        int64_t bw = 0;
        int ba = -1;
        for (uint32_t j = 0; j < k; ++j) {
            const uint64_t* ch = node(first + j);
            const uint32_t v = (uint32_t)ch[AT_VP];
            const int64_t w = (int64_t)ch[AT_W];
            const int a = (int)(flags(first + j) >> 8);
            visits[a] = (int32_t)v;
            if (value_sums) value_sums[a] = w;
            if (v > 0 && (ba < 0 || v > bv || (v == bv && w > bw))) {  // (no best while no child has a visit)
                ba = a;
                bv = v;
                bw = w;
            }
        }
        if (best) *best = ba;
    }

    // oth_puct_pick's move from the root's children: V the sum of their v (0: none, -1); not sampled:
    // outputs' best; sampled: the first child, in ascending squares, whose cumulative v exceeds
    // floor(u V / 2^32)
    OTH_HD int32_t pick_move(bool sample, uint32_t u) const {
        const uint64_t* root = node(0);
        const uint32_t first = (uint32_t)root[AT_LINK];
        const uint32_t k = first && (uint64_t)first + (uint32_t)root[AT_INFO] <= (uint64_t)used ? (uint32_t)root[AT_INFO] : 0u;
        uint64_t V = 0;
        for (uint32_t j = 0; j < k; ++j) V += (uint32_t)node(first + j)[AT_VP];
        if (V == 0) return -1;
        const uint64_t r = ((uint64_t)u * V) >> 32;
        uint64_t cum = 0;
        uint32_t bv = 0;
        int64_t bw = 0;
        int32_t ba = -1;
        for (uint32_t j = 0; j < k; ++j) {
            const uint64_t* ch = node(first + j);
            const uint32_t v = (uint32_t)ch[AT_VP];
            const int64_t w = (int64_t)ch[AT_W];
            const int32_t a = (int32_t)(flags(first + j) >> 8);
            if (sample) {
                cum += v;
                if (cum > r) return a;
            } else if (v > 0 && (ba < 0 || v > bv || (v == bv && w > bw))) {
                ba = a;
                bv = v;
                bw = w;
            }
        }
        return ba;
    }

    // The re-root's compaction in place, one sweep over the slots c .. used - 1: the subtree of c
    // moves to the slots 0 .. n - 1 in ascending order of the old indices and used = n.  A child's
    // index is above its parent's and a block of siblings is contiguous, so when the sweep reaches
    // a member it marks the member's children (F_KEEP; the first of them F_HEAD) and writes its own
    // new index into their parent halves: a slot above the sweep is never a target (a node's new
    // index is at most its old one), so the marks wait there untouched.  The first-child half of a
    // moved node is filled in when the sweep reaches that child (F_HEAD), through the parent's new
    // index.  The marks are cleared in the moved nodes; slots from n on are free and are written
    // whole before they are read again (apply).
    OTH_HD void compact(uint32_t c) {
        uint32_t n = 0;
        const uint32_t end = used;
        for (uint32_t i = c; i < end; ++i) {
            uint64_t* nd = node(i);
            const uint64_t info = nd[AT_INFO];
            const uint32_t f = (uint32_t)(info >> 32);
            if (i != c && !(f & F_KEEP)) continue;
            const uint32_t ni = n++;
            const uint64_t link = nd[AT_LINK];
            const uint32_t first = (uint32_t)link, k = (uint32_t)info;
            const uint32_t np = i == c ? 0u : (uint32_t)(link >> 32);  // (already the parent's new index)
            if (first != 0u && (uint64_t)first + k <= (uint64_t)end) {
                for (uint32_t j = 0; j < k; ++j) {
                    uint64_t* ch = node(first + j);
                    ch[AT_INFO] |= (uint64_t)(F_KEEP | (j == 0 ? F_HEAD : 0u)) << 32;
                    ch[AT_LINK] = (ch[AT_LINK] & 0xffffffffull) | (uint64_t)ni << 32;
                }
            }
            uint64_t* to = node(ni);
            for (int j = 0; j < AT_LINK; ++j) to[j] = nd[j];
            to[AT_LINK] = (uint64_t)np << 32;
            to[AT_INFO] = info & ~((uint64_t)(F_KEEP | F_HEAD) << 32);
            if (i != c && (f & F_HEAD)) node(np)[AT_LINK] |= (uint64_t)ni;
        }
        used = n;
    }
};

// The leaf arrays of board e after a call: the pending leaf, or (kind NONE) the root with the meta
// the handle held at begin; into the workspace's arrays and the caller's.
// (Ws: PuctWs<N>, row e = the board; or PuctBatchWs<N>, row e = board K + slot)
template <int N, class Ws>
OTH_HD void puct_write_leaf(const Ws& ws, size_t e, const PuctTree<N>& tr, uint32_t L, int kind,
                            uint32_t root_meta, const PuctLeaves& out) {
    constexpr int W = Geo<N>::W;
    BB<W> B, Wt, Lg;
    uint32_t meta;
    if (kind == PUCT_LEAF_NONE) {
        tr.position(0, B, Wt, Lg);
        meta = root_meta;
    } else {
        tr.leaf(L, B, Wt, Lg, meta);
    }
    uint64_t* lb = ws.leaf_boards() + e * 2 * W;
    uint64_t* ll = ws.leaf_legal() + e * W;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        lb[j] = B.w[j];
        lb[W + j] = Wt.w[j];
        ll[j] = Lg.w[j];
        if (out.boards) {
            out.boards[e * 2 * W + j] = B.w[j];
            out.boards[e * 2 * W + W + j] = Wt.w[j];
        }
        if (out.legal) out.legal[e * W + j] = Lg.w[j];
    }
    ws.leaf_meta()[e] = (uint16_t)meta;
    if (out.meta) out.meta[e] = (uint16_t)meta;
    if (out.kind) out.kind[e] = (uint8_t)kind;
}

// oth_puct_begin for board e (the handle's black, white, stored possible_moves and meta)
template <int N>
OTH_HD void puct_begin_board(const PuctWs<N>& ws, uint32_t e, const uint64_t* black, const uint64_t* white,
                             const uint64_t* stored, uint32_t meta, const PuctLeaves& out) {
    constexpr int W = Geo<N>::W;
    BB<W> B, Wt, Lg;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        B.w[i] = black[i];
        Wt.w[i] = white[i];
        Lg.w[i] = stored[i];
    }
    const int st = mcts_status<N>(Lg, meta);
    PuctTree<N> tr{ws.tree(e), 1u};
    tr.put_root(B, Wt, (meta & 1u) != 0, Lg & Geo<N>::BOARD);
    // (a stored mask of more than T - 1 squares, which no position of the game has, makes the root a VALUE leaf)
    const int kind = st == MCTS_DONE ? tr.leaf_kind(0, ws.T) : PUCT_LEAF_NONE;
    uint64_t* h = ws.hdr(e);
    h[0] = 1ull;  // used = 1, the pending leaf is the root
    h[1] = (uint64_t)(uint32_t)kind | (uint64_t)(uint32_t)st << 8 | (uint64_t)(meta & 0xffffu) << 32;
    puct_write_leaf<N>(ws, e, tr, 0u, kind, meta & 0xffffu, out);
}

// oth_puct_advance for board e.  priors: the board's N*N; the workspace is one that puct_begin_board wrote.
template <int N>
OTH_HD void puct_advance_board(const PuctWs<N>& ws, uint32_t e, int C, const int32_t* priors, int32_t value,
                               bool more, const PuctLeaves& out) {
    uint64_t* h = ws.hdr(e);
    const uint64_t h0 = h[0], h1 = h[1];
    PuctTree<N> tr{ws.tree(e), (uint32_t)h0};
    uint32_t L = (uint32_t)(h0 >> 32);
    int kind = (int)(h1 & 0xffu);
    if (tr.used > ws.T || L >= ws.T) kind = PUCT_LEAF_NONE, L = 0u;  // (a header no begin wrote: nothing is followed)
    if (kind != PUCT_LEAF_NONE) {
        tr.apply(L, kind, ws.T, priors, value);
        kind = PUCT_LEAF_NONE;
        L = 0u;
        if (more && (uint32_t)tr.node(0)[PuctTree<N>::AT_VP] < (uint32_t)PUCT_MAX_SIMS) L = tr.select(ws.T, C, kind);
        h[0] = (uint64_t)tr.used | (uint64_t)L << 32;
        h[1] = (h1 & ~0xffull) | (uint64_t)(uint32_t)kind;
    }
    puct_write_leaf<N>(ws, e, tr, L, kind, (uint32_t)(h1 >> 32), out);
}

// oth_puct_result for board e.  visits / value_sums: the board's N*N; value_sums, best, tree_nodes, status may be null.
template <int N>
OTH_HD void puct_result_board(const PuctWs<N>& ws, uint32_t e, int32_t* visits, int64_t* value_sums, int32_t* best,
                              int32_t* tree_nodes, uint8_t* status) {
    constexpr int NN = N * N;
    const uint64_t* h = ws.hdr(e);
    const uint32_t used = (uint32_t)h[0];
    const int st = (int)((h[1] >> 8) & 0xffu);
    if (status) *status = (uint8_t)st;
    if (st != MCTS_DONE || used > ws.T) {
        for (int a = 0; a < NN; ++a) {
            visits[a] = 0;
            if (value_sums) value_sums[a] = 0;
        }
        if (best) *best = -1;
        if (tree_nodes) *tree_nodes = 1;
        return;
    }
    const PuctTree<N> tr{ws.tree(e), used};
    tr.outputs(visits, value_sums, best);
    if (tree_nodes) *tree_nodes = (int32_t)used;
}

// oth_puct_pick for board e: the move of the search so far (id: the board's global env id + id_key)
template <int N>
OTH_HD int32_t puct_pick_board(const PuctWs<N>& ws, uint32_t e, bool sample, uint64_t seed, uint32_t id,
                               uint64_t counter) {
    const uint64_t* h = ws.hdr(e);
    const uint32_t used = (uint32_t)h[0];
    if ((int)((h[1] >> 8) & 0xffu) != MCTS_DONE || used > ws.T) return -1;
    const PuctTree<N> tr{ws.tree(e), used};
    return tr.pick_move(sample, sample ? philox4(seed, id, counter, PUCT_RNG_PICK).x : 0u);
}

// oth_puct_reroot for board e, in three steps that the device runs as three kernels (a lane, a
// wave, a lane per board) and puct_reroot_board one after the other.
//
// Step 1, the keep test against the handle's black, white, stored possible_moves and meta.  Kept:
// the header holds used | c << 32 and PUCT_REROOT_KEPT as its kind until step 3; not kept: the
// board is begun afresh from the handle's position (puct_begin_board, leaves included).
template <int N>
OTH_HD bool puct_reroot_classify(const PuctWs<N>& ws, uint32_t e, const uint64_t* black, const uint64_t* white,
                                 const uint64_t* stored, uint32_t meta, int32_t action, const PuctLeaves& out) {
    constexpr int W = Geo<N>::W;
    using Tree = PuctTree<N>;
    uint64_t* h = ws.hdr(e);
    const uint64_t h0 = h[0], h1 = h[1];
    const uint32_t used = (uint32_t)h0;
    bool keep = false;
    uint32_t c = 0;
    if ((int)((h1 >> 8) & 0xffu) == MCTS_DONE && used >= 1u && used <= ws.T && !(meta & 2u)) {
        const Tree tr{ws.tree(e), used};
        const uint64_t* root = tr.node(0);
        const uint32_t first = (uint32_t)root[Tree::AT_LINK], k = (uint32_t)root[Tree::AT_INFO];
        if (first != 0u && (uint64_t)first + k <= (uint64_t)used)
            for (uint32_t j = 0; j < k; ++j)
                if ((int32_t)(tr.flags(first + j) >> 8) == action) c = first + j;
        if (c != 0u) {
            if (!(tr.flags(c) & Tree::F_MADE)) tr.make(0u, c);
            BB<W> B, Wt, mv;
            tr.position(c, B, Wt, mv);
            const uint32_t f = tr.flags(c);
            keep = !(f & Tree::F_TERM) && ((f & Tree::F_TURN) != 0u) == ((meta & 1u) != 0u);
#pragma unroll
            for (int i = 0; i < W; ++i)
                keep = keep && B.w[i] == black[i] && Wt.w[i] == white[i] &&
                       mv.w[i] == (stored[i] & Geo<N>::BOARD.w[i]);
        }
    }
    if (!keep) {
        puct_begin_board<N>(ws, e, black, white, stored, meta, out);
        return false;
    }
    h[0] = (uint64_t)used | (uint64_t)c << 32;
    h[1] = (uint64_t)PUCT_REROOT_KEPT | (uint64_t)(uint32_t)MCTS_DONE << 8 | (uint64_t)(meta & 0xffffu) << 32;
    return true;
}

// Step 2 on one lane: the compaction of a kept board (PuctTree::compact)
template <int N>
OTH_HD void puct_reroot_sweep(const PuctWs<N>& ws, uint32_t e) {
    uint64_t* h = ws.hdr(e);
    const uint64_t h0 = h[0];
    if ((h[1] & 0xffu) != (uint64_t)PUCT_REROOT_KEPT) return;
    PuctTree<N> tr{ws.tree(e), (uint32_t)h0};
    tr.compact((uint32_t)(h0 >> 32));
    h[0] = (uint64_t)tr.used;
}

// step 4 of the re-root: the new priors of a kept root's children (root_priors: the board's N*N, may be null)
template <int N>
OTH_HD void puct_root_priors(const PuctTree<N>& tr, const int32_t* root_priors) {
    using Tree = PuctTree<N>;
    const uint64_t* root = tr.node(0);
    const uint32_t first = (uint32_t)root[Tree::AT_LINK], k = (uint32_t)root[Tree::AT_INFO];
    if (root_priors && first != 0u) {
        for (uint32_t j = 0; j < k; ++j) {
            uint64_t* ch = tr.node(first + j);
            const int32_t pr = root_priors[tr.flags(first + j) >> 8];
            const uint32_t P = (uint32_t)(pr < 0 ? 0 : (pr > PUCT_PRIOR_MAX ? PUCT_PRIOR_MAX : pr));
            ch[Tree::AT_VP] = (ch[Tree::AT_VP] & 0xffffffffull) | (uint64_t)P << 32;
        }
    }
}

// Step 3: a kept root's new priors (root_priors: the board's N*N, may be null), its selection and the leaves
template <int N>
OTH_HD void puct_reroot_finish(const PuctWs<N>& ws, uint32_t e, int C, const int32_t* root_priors, uint8_t* kept,
                               const PuctLeaves& out) {
    using Tree = PuctTree<N>;
    uint64_t* h = ws.hdr(e);
    const uint64_t h1 = h[1];
    const bool keep = (h1 & 0xffu) == (uint64_t)PUCT_REROOT_KEPT;
    if (kept) *kept = keep ? 1 : 0;
    if (!keep) return;
    const Tree tr{ws.tree(e), (uint32_t)h[0]};
    const uint64_t* root = tr.node(0);
    puct_root_priors<N>(tr, root_priors);
    int kind = PUCT_LEAF_NONE;
    uint32_t L = 0u;
    if ((uint32_t)root[Tree::AT_VP] < (uint32_t)PUCT_MAX_SIMS) L = tr.select(ws.T, C, kind);
    h[0] = (uint64_t)tr.used | (uint64_t)L << 32;
    h[1] = (h1 & ~0xffull) | (uint64_t)(uint32_t)kind;
    puct_write_leaf<N>(ws, e, tr, L, kind, (uint32_t)(h1 >> 32), out);
}

// oth_puct_reroot for board e: the spec of the call, and the device's one-lane mapping
template <int N>
OTH_HD void puct_reroot_board(const PuctWs<N>& ws, uint32_t e, int C, const uint64_t* black, const uint64_t* white,
                              const uint64_t* stored, uint32_t meta, int32_t action, const int32_t* root_priors,
                              uint8_t* kept, const PuctLeaves& out) {
    if (puct_reroot_classify<N>(ws, e, black, white, stored, meta, action, out)) puct_reroot_sweep<N>(ws, e);
    puct_reroot_finish<N>(ws, e, C, root_priors, kept, out);
}

// ---- the batch calls: K slots a board, row e K + j of the leaf arrays is slot j of board e ----

// The leaves of board e's K slots after a batch call, into the extension's arrays and the caller's
template <int N>
OTH_HD void puct_write_slots(const PuctBatchWs<N>& bw, uint32_t e, const PuctTree<N>& tr, uint32_t root_meta,
                             const PuctLeaves& out) {
    const uint64_t* sl = bw.slots(e);
    for (uint32_t j = 0; j < bw.K; ++j)
        puct_write_leaf<N>(bw, (size_t)e * bw.K + j, tr, (uint32_t)sl[j], (int)(sl[j] >> 32), root_meta, out);
}

// The Select of a batch call for board e (a DONE board's tree): slot after slot in ascending order under
// the launch's virtual loss, which is taken out again before the function returns
template <int N>
OTH_HD void puct_select_slots(const PuctBatchWs<N>& bw, uint32_t e, const PuctTree<N>& tr, int C, uint32_t sim_limit) {
    uint64_t* sl = bw.slots(e);
    const uint32_t v0 = (uint32_t)tr.node(0)[PuctTree<N>::AT_VP];
    uint32_t r = tr.used;
    bool open = true;
    for (uint32_t j = 0; j < bw.K; ++j) {
        uint32_t L = 0u;
        int kind = PUCT_LEAF_NONE;
        if (open && (uint64_t)v0 + j < (uint64_t)sim_limit) {
            L = tr.select_vl(bw.plain.T, C, r, kind);
            if (kind == PUCT_LEAF_NONE) L = 0u, open = false;  // a collision closes the board for this launch
            else if (j + 1u < bw.K) tr.count_path(L, 1);      // (no slot reads the last one's path)
        }
        sl[j] = (uint64_t)L | (uint64_t)(uint32_t)kind << 32;
    }
    for (uint32_t j = 0; j + 1u < bw.K; ++j)
        if ((uint32_t)(sl[j] >> 32) != (uint32_t)PUCT_LEAF_NONE) tr.count_path((uint32_t)sl[j], -1);
}

// oth_puct_begin_batch for board e: puct_begin_board, the root as slot 0's leaf
template <int N>
OTH_HD void puct_begin_batch_board(const PuctBatchWs<N>& bw, uint32_t e, const uint64_t* black, const uint64_t* white,
                                   const uint64_t* stored, uint32_t meta, const PuctLeaves& out) {
    const PuctWs<N>& ws = bw.plain;
    puct_begin_board<N>(ws, e, black, white, stored, meta, PuctLeaves{nullptr, nullptr, nullptr, nullptr});
    uint64_t* h = ws.hdr(e);
    const uint64_t h1 = h[1];
    uint64_t* sl = bw.slots(e);
    sl[0] = (h1 & 0xffull) << 32;
    for (uint32_t j = 1; j < bw.K; ++j) sl[j] = 0ull;
    h[1] = h1 & ~0xffull;  // (kind NONE in the header: a plain advance does nothing to this board)
    puct_write_slots<N>(bw, e, PuctTree<N>{ws.tree(e), 1u}, (uint32_t)(h1 >> 32), out);
}

// oth_puct_advance_batch for board e.  priors: the board's K rows of N*N; values: its K
template <int N>
OTH_HD void puct_advance_batch_board(const PuctBatchWs<N>& bw, uint32_t e, int C, const int32_t* priors,
                                     const int32_t* values, uint32_t sim_limit, const PuctLeaves& out) {
    const PuctWs<N>& ws = bw.plain;
    uint64_t* h = ws.hdr(e);
    const uint64_t h1 = h[1];
    PuctTree<N> tr{ws.tree(e), (uint32_t)h[0]};
    uint64_t* sl = bw.slots(e);
    bool any = false;
    for (uint32_t j = 0; j < bw.K; ++j) {  // Apply, in slot order
        const uint32_t L = (uint32_t)sl[j];
        const int kind = (int)(sl[j] >> 32);
        if (kind < PUCT_LEAF_EXPAND || kind > PUCT_LEAF_TERMINAL || L >= tr.used || tr.used > ws.T) {
            sl[j] = 0ull;  // (no leaf; or a slot no batch call wrote: nothing is followed)
            continue;
        }
        tr.apply(L, kind, ws.T, priors + (size_t)j * (N * N), values[j]);
        any = true;
    }
    if (any) {
        puct_select_slots<N>(bw, e, tr, C, sim_limit);
        h[0] = (uint64_t)tr.used;
    }
    puct_write_slots<N>(bw, e, tr, (uint32_t)(h1 >> 32), out);
}

// oth_puct_reroot_batch's step after puct_reroot_classify and the sweep: the slots' leaves are
// discarded, a kept root takes its new priors, and a DONE board, kept or fresh, runs the Select
template <int N>
OTH_HD void puct_reroot_finish_batch(const PuctBatchWs<N>& bw, uint32_t e, int C, const int32_t* root_priors,
                                     uint8_t* kept, uint32_t sim_limit, const PuctLeaves& out) {
    const PuctWs<N>& ws = bw.plain;
    uint64_t* h = ws.hdr(e);
    const uint64_t h1 = h[1];
    const bool keep = (h1 & 0xffu) == (uint64_t)PUCT_REROOT_KEPT;
    if (kept) *kept = keep ? 1 : 0;
    const PuctTree<N> tr{ws.tree(e), (uint32_t)h[0]};
    uint64_t* sl = bw.slots(e);
    for (uint32_t j = 0; j < bw.K; ++j) sl[j] = 0ull;
    if (keep) puct_root_priors<N>(tr, root_priors);
    if ((int)((h1 >> 8) & 0xffu) == MCTS_DONE && tr.used >= 1u && tr.used <= ws.T)
        puct_select_slots<N>(bw, e, tr, C, sim_limit);
    h[0] = (uint64_t)tr.used;
    h[1] = h1 & ~0xffull;
    puct_write_slots<N>(bw, e, tr, (uint32_t)(h1 >> 32), out);
}

// oth_puct_reroot_batch for board e: the spec of the call
template <int N>
OTH_HD void puct_reroot_batch_board(const PuctBatchWs<N>& bw, uint32_t e, int C, const uint64_t* black,
                                    const uint64_t* white, const uint64_t* stored, uint32_t meta, int32_t action,
                                    const int32_t* root_priors, uint8_t* kept, uint32_t sim_limit,
                                    const PuctLeaves& out) {
    if (puct_reroot_classify<N>(bw.plain, e, black, white, stored, meta, action,
                                PuctLeaves{nullptr, nullptr, nullptr, nullptr}))
        puct_reroot_sweep<N>(bw.plain, e);
    puct_reroot_finish_batch<N>(bw, e, C, root_priors, kept, sim_limit, out);
}

}  // namespace oth

#if defined(__HIPCC__)
#include "state.hpp"

namespace oth_dev {

static_assert(PUCT_VALUE_ONE == OTH_PUCT_VALUE_ONE && PUCT_PRIOR_MAX == OTH_PUCT_PRIOR_MAX &&
                  PUCT_MAX_C == OTH_PUCT_MAX_C && PUCT_MAX_TREE_NODES == OTH_PUCT_MAX_TREE_NODES &&
                  PUCT_MAX_SIMS == OTH_PUCT_MAX_SIMS && PUCT_MAX_LEAVES == OTH_PUCT_MAX_LEAVES,
              "the header's limits");
static_assert(PUCT_LEAF_NONE == OTH_PUCT_LEAF_NONE && PUCT_LEAF_EXPAND == OTH_PUCT_LEAF_EXPAND &&
                  PUCT_LEAF_VALUE == OTH_PUCT_LEAF_VALUE && PUCT_LEAF_TERMINAL == OTH_PUCT_LEAF_TERMINAL,
              "the header's leaf kinds");
static_assert(PUCT_RNG_PICK == RNG_PUCT_PICK, "state.hpp's purpose word");
static_assert(OTH_PUCT_REROOT_LDS >= 64 && OTH_PUCT_REROOT_LDS <= 16384, "the forwarding table's share of the LDS");

constexpr int PUCT_BLOCK = 64;  // one wave a block, one lane a board

template <int N>
__global__ __launch_bounds__(PUCT_BLOCK) void k_puct_begin(const uint64_t* __restrict__ boards,
                                                           const uint16_t* __restrict__ meta,
                                                           const uint64_t* __restrict__ legal, int E, uint32_t T,
                                                           uint64_t* __restrict__ wsp, PuctLeaves out) {
    constexpr int W = Geo<N>::W;
    const long long e = (long long)blockIdx.x * PUCT_BLOCK + threadIdx.x;
    const PuctWs<N> ws{wsp, (uint32_t)E, T};
    if (e == 0) *ws.tag() = puct_tag(N, (uint32_t)E, T);
    if (e >= E) return;
    puct_begin_board<N>(ws, (uint32_t)e, boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W,
                        legal + (size_t)e * W, meta[e], out);
}

// (a workspace whose tag is not this search's -- no begin for this handle and T -- is left alone)
template <int N>
__global__ __launch_bounds__(PUCT_BLOCK) void k_puct_advance(int E, uint32_t T, int C, uint64_t* __restrict__ wsp,
                                                             const int32_t* __restrict__ priors,
                                                             const int32_t* __restrict__ values, int more,
                                                             PuctLeaves out) {
    const long long e = (long long)blockIdx.x * PUCT_BLOCK + threadIdx.x;
    const PuctWs<N> ws{wsp, (uint32_t)E, T};
    if (e >= E || *ws.tag() != puct_tag(N, (uint32_t)E, T)) return;
    puct_advance_board<N>(ws, (uint32_t)e, C, priors + (size_t)e * (N * N), values[e], more != 0, out);
}

template <int N>
__global__ __launch_bounds__(PUCT_BLOCK) void k_puct_result(int E, uint32_t T, uint64_t* __restrict__ wsp,
                                                            int32_t* __restrict__ visits,
                                                            int64_t* __restrict__ value_sums,
                                                            int32_t* __restrict__ best,
                                                            int32_t* __restrict__ tree_nodes,
                                                            uint8_t* __restrict__ status) {
    constexpr int NN = N * N;
    const long long e = (long long)blockIdx.x * PUCT_BLOCK + threadIdx.x;
    const PuctWs<N> ws{wsp, (uint32_t)E, T};
    if (e >= E || *ws.tag() != puct_tag(N, (uint32_t)E, T)) return;
    puct_result_board<N>(ws, (uint32_t)e, visits + (size_t)e * NN, value_sums ? value_sums + (size_t)e * NN : nullptr,
                         best ? best + e : nullptr, tree_nodes ? tree_nodes + e : nullptr,
                         status ? status + e : nullptr);
}

template <int N>
__global__ __launch_bounds__(PUCT_BLOCK) void k_puct_pick(int E, uint32_t T, uint64_t* __restrict__ wsp,
                                                          const uint8_t* __restrict__ sample, uint64_t seed,
                                                          uint32_t id0, uint64_t counter,
                                                          int32_t* __restrict__ actions) {
    const long long e = (long long)blockIdx.x * PUCT_BLOCK + threadIdx.x;
    const PuctWs<N> ws{wsp, (uint32_t)E, T};
    if (e >= E || *ws.tag() != puct_tag(N, (uint32_t)E, T)) return;
    actions[e] = puct_pick_board<N>(ws, (uint32_t)e, sample && sample[e] != 0, seed, id0 + (uint32_t)e, counter);
}

// oth_puct_reroot, the one-lane mapping: the whole call of a board on its lane (OTH_PUCT_REROOT_LANE)
template <int N>
__global__ __launch_bounds__(PUCT_BLOCK) void k_puct_reroot_lane(const uint64_t* __restrict__ boards,
                                                                 const uint16_t* __restrict__ meta,
                                                                 const uint64_t* __restrict__ legal, int E, uint32_t T,
                                                                 int C, uint64_t* __restrict__ wsp,
                                                                 const int32_t* __restrict__ actions,
                                                                 const int32_t* __restrict__ root_priors,
                                                                 uint8_t* __restrict__ kept, PuctLeaves out) {
    constexpr int W = Geo<N>::W;
    const long long e = (long long)blockIdx.x * PUCT_BLOCK + threadIdx.x;
    const PuctWs<N> ws{wsp, (uint32_t)E, T};
    if (e >= E || *ws.tag() != puct_tag(N, (uint32_t)E, T)) return;
    puct_reroot_board<N>(ws, (uint32_t)e, C, boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W,
                         legal + (size_t)e * W, meta[e], actions[e],
                         root_priors ? root_priors + (size_t)e * (N * N) : nullptr, kept ? kept + e : nullptr, out);
}

// oth_puct_reroot, the shipped mapping, in three launches: the keep test on a lane per board ...
template <int N>
__global__ __launch_bounds__(PUCT_BLOCK) void k_puct_reroot_classify(const uint64_t* __restrict__ boards,
                                                                     const uint16_t* __restrict__ meta,
                                                                     const uint64_t* __restrict__ legal, int E,
                                                                     uint32_t T, uint64_t* __restrict__ wsp,
                                                                     const int32_t* __restrict__ actions,
                                                                     PuctLeaves out) {
    constexpr int W = Geo<N>::W;
    const long long e = (long long)blockIdx.x * PUCT_BLOCK + threadIdx.x;
    const PuctWs<N> ws{wsp, (uint32_t)E, T};
    if (e >= E || *ws.tag() != puct_tag(N, (uint32_t)E, T)) return;
    puct_reroot_classify<N>(ws, (uint32_t)e, boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W,
                            legal + (size_t)e * W, meta[e], actions[e], out);
}

// ... the compaction on a wave per board (block e is board e; a board that is not kept returns at
// once).  A lane takes one of 64 consecutive slots, from c on.  Pass 1 reads the slots' link words
// and fills the forwarding table in LDS, fwd[old - c] = the new index or NONE: a slot is a member
// if its parent is -- from the table when the parent lies in an earlier chunk, by propagating the
// ballot of the members over the wave until it is stable when it lies in the same chunk (a
// parent's index is below its child's, so every round decides the lowest open lane at least) --
// and the new index is the members before the chunk plus the ballot's prefix.  Pass 2 reads the
// members' nodes into registers, translates both halves of the link word through the table and
// stores them at their new slots: a new index is at most the old one, so a chunk's targets lie
// below the next chunk's sources, and within a chunk every source word is in registers (the
// counter of outstanding loads drained) before the first store.  A subtree of more than
// OTH_PUCT_REROOT_LDS slots is compacted in place by lane 0 (PuctTree::compact).
template <int N>
__device__ __forceinline__ void puct_sweep_wave(const PuctWs<N>& ws, uint32_t* fwd) {
    using Tree = PuctTree<N>;
    constexpr int WORDS = Tree::WORDS;
    constexpr uint32_t NONE = 0xffffffffu;
    const uint32_t e = blockIdx.x, lane = threadIdx.x;
    const uint32_t T = ws.T;
    uint64_t* h = ws.hdr(e);
    const uint64_t h0 = h[0];
    if ((h[1] & 0xffu) != (uint64_t)PUCT_REROOT_KEPT) return;  // (the same for the whole wave)
    const uint32_t used = (uint32_t)h0, c = (uint32_t)(h0 >> 32);
    if (c == 0u || c >= used || used > T) return;  // (no classify wrote this)
    if (used - c > (uint32_t)OTH_PUCT_REROOT_LDS) {
        if (lane == 0) puct_reroot_sweep<N>(ws, e);
        return;
    }
    uint64_t* t = ws.tree(e);
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t n = 0;  // members before the chunk
    for (uint32_t b = c; b < used; b += 64u) {
        const uint32_t i = b + lane;
        const bool valid = i < used;
        const uint32_t p = valid ? (uint32_t)(t[(size_t)i * WORDS + Tree::AT_LINK] >> 32) : 0u;
        bool known = true, mem = false;
        if (valid) {
            if (i == c) mem = true;
            else if (p < c || p >= i) mem = false;  // (p >= i: no tree has it)
            else if (p < b) mem = fwd[p - c] != NONE;
            else known = false;  // the parent is a lower lane of this chunk
        }
        for (;;) {
            const uint64_t bk = __ballot(known), bm = __ballot(mem);
            if (bk == ~0ull) break;
            if (!known && ((bk >> (p - b)) & 1ull)) {
                mem = ((bm >> (p - b)) & 1ull) != 0ull;
                known = true;
            }
        }
        const uint64_t bm = __ballot(mem);
        if (valid) fwd[i - c] = mem ? n + (uint32_t)__popcll(bm & below) : NONE;
        n += (uint32_t)__popcll(bm);
        __syncthreads();
    }
    for (uint32_t b = c; b < used; b += 64u) {
        const uint32_t i = b + lane;
        const uint32_t ni = i < used ? fwd[i - c] : NONE;
        uint64_t w[WORDS];
        if (ni != NONE) {
            const uint64_t* nd = t + (size_t)i * WORDS;
#pragma unroll
            for (int j = 0; j < WORDS; ++j) w[j] = nd[j];
            const uint32_t first = (uint32_t)w[Tree::AT_LINK], p = (uint32_t)(w[Tree::AT_LINK] >> 32);
            const uint32_t np = i == c ? 0u : fwd[p - c];
            const uint32_t nf = first > i && first < used ? fwd[first - c] : 0u;
            w[Tree::AT_LINK] = (uint64_t)nf | (uint64_t)np << 32;
        }
        __builtin_amdgcn_s_waitcnt(0);  // every lane's loads of this chunk have returned
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        if (ni != NONE) {
            uint64_t* to = t + (size_t)ni * WORDS;
#pragma unroll
            for (int j = 0; j < WORDS; ++j) to[j] = w[j];
        }
    }
    if (lane == 0) h[0] = (uint64_t)n;
}

template <int N>
__global__ __launch_bounds__(64) void k_puct_reroot_sweep(int E, uint32_t T, uint64_t* wsp) {
    __shared__ uint32_t fwd[OTH_PUCT_REROOT_LDS];
    const PuctWs<N> ws{wsp, (uint32_t)E, T};
    if (*ws.tag() != puct_tag(N, (uint32_t)E, T)) return;
    puct_sweep_wave<N>(ws, fwd);
}

// ... and the new priors, the selection and the leaves on a lane per board
template <int N>
__global__ __launch_bounds__(PUCT_BLOCK) void k_puct_reroot_finish(int E, uint32_t T, int C,
                                                                   uint64_t* __restrict__ wsp,
                                                                   const int32_t* __restrict__ root_priors,
                                                                   uint8_t* __restrict__ kept, PuctLeaves out) {
    const long long e = (long long)blockIdx.x * PUCT_BLOCK + threadIdx.x;
    const PuctWs<N> ws{wsp, (uint32_t)E, T};
    if (e >= E || *ws.tag() != puct_tag(N, (uint32_t)E, T)) return;
    puct_reroot_finish<N>(ws, (uint32_t)e, C, root_priors ? root_priors + (size_t)e * (N * N) : nullptr,
                          kept ? kept + e : nullptr, out);
}

// ---- the batch calls (oth_puct_begin_batch / _advance_batch / _reroot_batch): a lane per board runs the
// board's K slots one after the other -- the selection is sequential by definition -- so, as in the plain
// calls, one lane owns every word of its board, its slots and its K rows of leaves.  (A workspace that no
// begin_batch of this geometry, T and K wrote is left alone.)

template <int N>
__global__ __launch_bounds__(PUCT_BLOCK) void k_puct_begin_batch(const uint64_t* __restrict__ boards,
                                                                 const uint16_t* __restrict__ meta,
                                                                 const uint64_t* __restrict__ legal, int E, uint32_t T,
                                                                 uint32_t K, uint64_t* __restrict__ wsp,
                                                                 PuctLeaves out) {
    constexpr int W = Geo<N>::W;
    const long long e = (long long)blockIdx.x * PUCT_BLOCK + threadIdx.x;
    const PuctBatchWs<N> bw{PuctWs<N>{wsp, (uint32_t)E, T}, K};
    if (e == 0) bw.put_tags();
    if (e >= E) return;
    puct_begin_batch_board<N>(bw, (uint32_t)e, boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W,
                              legal + (size_t)e * W, meta[e], out);
}

template <int N>
__global__ __launch_bounds__(PUCT_BLOCK) void k_puct_advance_batch(int E, uint32_t T, uint32_t K, int C,
                                                                   uint64_t* __restrict__ wsp,
                                                                   const int32_t* __restrict__ priors,
                                                                   const int32_t* __restrict__ values,
                                                                   uint32_t sim_limit, PuctLeaves out) {
    const long long e = (long long)blockIdx.x * PUCT_BLOCK + threadIdx.x;
    const PuctBatchWs<N> bw{PuctWs<N>{wsp, (uint32_t)E, T}, K};
    if (e >= E || !bw.begun()) return;
    puct_advance_batch_board<N>(bw, (uint32_t)e, C, priors + (size_t)e * K * (N * N), values + (size_t)e * K, sim_limit,
                                out);
}

// oth_puct_reroot_batch in three launches, as oth_puct_reroot: the keep test (it writes no leaves: a fresh
// board's come with the finish) ...
template <int N>
__global__ __launch_bounds__(PUCT_BLOCK) void k_puct_reroot_classify_batch(const uint64_t* __restrict__ boards,
                                                                           const uint16_t* __restrict__ meta,
                                                                           const uint64_t* __restrict__ legal, int E,
                                                                           uint32_t T, uint32_t K,
                                                                           uint64_t* __restrict__ wsp,
                                                                           const int32_t* __restrict__ actions) {
    constexpr int W = Geo<N>::W;
    const long long e = (long long)blockIdx.x * PUCT_BLOCK + threadIdx.x;
    const PuctBatchWs<N> bw{PuctWs<N>{wsp, (uint32_t)E, T}, K};
    if (e >= E || !bw.begun()) return;
    puct_reroot_classify<N>(bw.plain, (uint32_t)e, boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W,
                            legal + (size_t)e * W, meta[e], actions[e], PuctLeaves{nullptr, nullptr, nullptr, nullptr});
}

// ... the compaction, k_puct_reroot_sweep's wave per board ...
template <int N>
__global__ __launch_bounds__(64) void k_puct_reroot_sweep_batch(int E, uint32_t T, uint32_t K, uint64_t* wsp) {
    __shared__ uint32_t fwd[OTH_PUCT_REROOT_LDS];
    const PuctBatchWs<N> bw{PuctWs<N>{wsp, (uint32_t)E, T}, K};
    if (!bw.begun()) return;
    puct_sweep_wave<N>(bw.plain, fwd);
}

// ... and the new priors, the Select and the leaves on a lane per board
template <int N>
__global__ __launch_bounds__(PUCT_BLOCK) void k_puct_reroot_finish_batch(int E, uint32_t T, uint32_t K, int C,
                                                                         uint64_t* __restrict__ wsp,
                                                                         const int32_t* __restrict__ root_priors,
                                                                         uint8_t* __restrict__ kept,
                                                                         uint32_t sim_limit, PuctLeaves out) {
    const long long e = (long long)blockIdx.x * PUCT_BLOCK + threadIdx.x;
    const PuctBatchWs<N> bw{PuctWs<N>{wsp, (uint32_t)E, T}, K};
    if (e >= E || !bw.begun()) return;
    puct_reroot_finish_batch<N>(bw, (uint32_t)e, C, root_priors ? root_priors + (size_t)e * (N * N) : nullptr,
                                kept ? kept + e : nullptr, sim_limit, out);
}

}  // namespace oth_dev
#endif
