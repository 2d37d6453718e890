// policy.hpp -- the scripted policies' moves: MaxiMin (compile-time and runtime
// depth) and policy_action, the move of any deterministic policy.
#pragma once
#include "engines.hpp"

namespace oth_dev {

// MaxiMinPolicy(depth).get_action (simple_policies.py:98-163).  P is the side to
// move at this node, O the other side; the root mover's ("my") discs are P at
// even levels and O at odd ones.  A child is a leaf when the search depth is
// reached, the board is full, or the side to reply has no move: the
// reference then either ends the game (double pass) or forces the turn to
// that side anyway (:139-144), whose empty move list ends the branch
// (:117-126) -- either way the leaf value is my disc count.  Ties keep the
// first (lowest) square: np.argmax / np.argmin (:152-154).  The depth is a
// template parameter, so the recursion unrolls into straight-line levels.
template <int N, int D, int LVL>
__device__ int maximin_node(const BB<Geo<N>::W>& P, const BB<Geo<N>::W>& O, const BB<Geo<N>::W>& L, int& move) {
    constexpr int W = Geo<N>::W;
    constexpr bool MINE = (LVL % 2) == 0;
    int best = MINE ? -1 : 0x7fffffff;
    move = -1;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        uint64_t x = L.w[i];
        while (x) {
            const int b = __builtin_ctzll(x);
            x &= x - 1;
            BB<W> m = zero<W>();
            m.w[i] = 1ull << b;
            const BB<W> f = flips<N>(P, O, m);
            const BB<W> P2 = P | f | m;
            const BB<W> O2 = O & ~(f | m);
            int v = popcount(MINE ? P2 : O2);
            if constexpr (LVL + 2 == D) {
                // the child is the last level: its value is the mover's best flip
                // count over its moves (bit planes, no loop): my discs after the
                // child's move are O2 + flips + 1 when I move there, P2 - flips otherwise
                if (any(~(P2 | O2) & Geo<N>::BOARD)) {
                    BB<W> t2[8];
                    const BB<W> L2 = legal_moves_fills<N>(O2, P2, t2);
                    if (any(L2)) {
                        const int mf = PlanesW<N>::max_flips(t2, L2);
                        v = ((LVL + 1) % 2 == 0) ? popcount(O2) + 1 + mf : popcount(P2) - mf;
                    }
                }
            } else if constexpr (LVL + 1 < D) {
                if (any(~(P2 | O2) & Geo<N>::BOARD)) {
                    const BB<W> L2 = legal_moves<N>(O2, P2);
                    if (any(L2)) {
                        int unused;
                        v = maximin_node<N, D, LVL + 1>(O2, P2, L2, unused);
                    }
                }
            }
            if (MINE ? v > best : v < best) {
                best = v;
                move = 64 * i + b;
            }
        }
    }
    return best;
}

// MaxiMinPolicy(D).get_action for a runtime depth D (the OTH_POLICY_MAXIMIN_DEEP
// launches, D >= 4; maximin_node's rules): the reference's recursion
// (simple_policies.py:111-155) as a depth-first walk over an explicit stack,
// one level per search depth -- level l moves the root's side at even l and
// holds (mover, other, moves not yet tried, best value, move being tried).
// The level above the leaves takes its value from the greedy planes' maximum
// flip count, as maximin_node does.  -1 without a move (the reference's None).
template <int N>
__device__ int maximin_search(const BB<Geo<N>::W>& P0, const BB<Geo<N>::W>& O0, const BB<Geo<N>::W>& L0, int D) {
    constexpr int W = Geo<N>::W;
    constexpr int MAXD = OTH_MAXIMIN_MAX_DEPTH;
    BB<W> SP[MAXD], SO[MAXD], SR[MAXD];
    int SV[MAXD], SM[MAXD];
    if (!any(L0)) return -1;
    int best_move = -1, l = 0;
    SP[0] = P0;
    SO[0] = O0;
    SR[0] = L0;
    SV[0] = -1;
    for (;;) {
        if (!any(SR[l])) {  // every move of level l tried: its value goes to the level above
            if (l == 0) break;
            const int v = SV[l];
            --l;
            if ((l & 1) == 0 ? v > SV[l] : v < SV[l]) {  // np.argmax / np.argmin: the first of equals
                SV[l] = v;
                if (l == 0) best_move = SM[l];
            }
            continue;
        }
        // the lowest untried move of level l (possible_moves ascending)
        BB<W> R = SR[l], m = zero<W>();
        int b = -1;
#pragma unroll
        for (int i = W - 1; i >= 0; --i)
            if (R.w[i]) b = 64 * i + ctz64(R.w[i]);
#pragma unroll
        for (int i = 0; i < W; ++i) {
            m.w[i] = (b >> 6) == i ? 1ull << (b & 63) : 0ull;
            R.w[i] &= ~m.w[i];
        }
        SR[l] = R;
        SM[l] = b;
        const BB<W> P = SP[l], O = SO[l];
        const BB<W> f = flips<N>(P, O, m);
        const BB<W> P2 = P | f | m;
        const BB<W> O2 = O & ~(f | m);
        const bool mine = (l & 1) == 0;
        int v = popcount(mine ? P2 : O2);  // a leaf: my disc count (:117-126)
        bool leaf = true;
        if (l + 1 < D && any(~(P2 | O2) & Geo<N>::BOARD)) {
            BB<W> t2[8];
            const BB<W> L2 = legal_moves_fills<N>(O2, P2, t2);
            if (any(L2)) {  // no reply: the game ends or the turn is forced back to a side without moves
                if (l + 2 == D) {  // the child's moves end the search: its best from the planes
                    const int mf = PlanesW<N>::max_flips(t2, L2);
                    v = ((l + 1) & 1) == 0 ? popcount(O2) + 1 + mf : popcount(P2) - mf;
                } else {
                    ++l;
                    SP[l] = O2;
                    SO[l] = P2;
                    SR[l] = L2;
                    SV[l] = (l & 1) == 0 ? -1 : 0x7fffffff;
                    leaf = false;
                }
            }
        }
        if (leaf && (mine ? v > SV[l] : v < SV[l])) {
            SV[l] = v;
            if (l == 0) best_move = b;
        }
    }
    return best_move;
}

template <int N, int D>
__device__ __forceinline__ int maximin_action(const Lane<N>& s) {
    const bool tw = (s.meta & M_TURN_WHITE) != 0;
    int move;
    maximin_node<N, D, 0>(pick(tw, s.white, s.black), pick(tw, s.black, s.white), s.legal, move);
    return move;
}

// The move of a deterministic scripted policy (everything but RANDOM); depth:
// the search depth of OTH_POLICY_MAXIMIN_DEEP (Rng::depth).
constexpr int OTH_POLICY_MAXIMIN_DEEP = 0x100;  // launcher-internal: MaxiMin of a runtime depth >= 4
template <int N, int POLICY, typename Eng>
__device__ __forceinline__ int policy_action(const Lane<N>& s, const Eng& eng, int depth = 0) {
    if constexpr (POLICY == OTH_POLICY_GREEDY) {
        return greedy_action<N>(s, eng);
    } else if constexpr (POLICY == OTH_POLICY_MAXIMIN2) {
        return maximin_action<N, 2>(s);
    } else if constexpr (POLICY == OTH_POLICY_MAXIMIN3) {
        return maximin_action<N, 3>(s);
    } else if constexpr (POLICY == OTH_POLICY_MAXIMIN_DEEP) {
        const bool tw = (s.meta & M_TURN_WHITE) != 0;
        return maximin_search<N>(pick(tw, s.white, s.black), pick(tw, s.black, s.white), s.legal, depth);
    } else {
        return -1;
    }
}

}  // namespace oth_dev
