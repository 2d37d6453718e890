// ntuple.hpp -- oth_ntuple_*: the n-tuple network (the spec is the header's comment on
// oth_ntuple_eval: a sum of look-up tables indexed by the contents of small sets of squares,
// applied under the eight board symmetries, trained by a delta rule; every output is an exact
// integer function of the row, the parameters and the weights) and oth_search_ntuple, oth_search
// with that value at the frontier.
//
// The part outside __HIPCC__ is plain host/device code: the parameter check, the plan (the 8 T
// transformed square lists and the tables' offsets as an address-free blob of 32-bit words), the
// cell code, index, sum, value and delta of one row, and the search's node step (search_step with
// another leaf rule; root_tasks.hpp and SearchFrame as they are).  tests/host/ntuple_host.cpp
// compiles it with g++; ntuple_n.hip's kernels run the same text.
//
// The plan, in 32-bit words: a header of NTUPLE_HEAD words -- a tag, the board size, T,
// value_shift, n_weights, a hash of the lengths and squares, the plan's words, 0 -- then per tuple
// NTUPLE_REC words: its table's offset, its length, and per symmetry s two words holding
// sigma_s(q_{t,i}) as byte i.  A square is below 256, so a list of 8 takes two words and the whole
// plan at most 8 + 32 * 18 words = 2,336 bytes.
#pragma once
#include "search.hpp"

namespace oth {

constexpr int NTUPLE_MAX_TUPLES = 32, NTUPLE_MAX_LENGTH = 8, NTUPLE_MAX_SHIFT = 24;
constexpr int NTUPLE_MAX_ROWS = 1 << 24, NTUPLE_MAX_RATE = 1 << 24, NTUPLE_MAX_RATE_SHIFT = 40;
constexpr int NTUPLE_DELTA_MAX = 1 << 30, NTUPLE_VALUE_ONE = 32768;
constexpr int NTUPLE_HEAD = 8, NTUPLE_REC = 18;
constexpr uint32_t NTUPLE_TAG = 0x4c50544eu;  // "NTPL"

// struct oth_ntuple_params, field for field
struct NtupleParams {
    int32_t tuples;
    int32_t length[NTUPLE_MAX_TUPLES];
    int32_t squares[NTUPLE_MAX_TUPLES][NTUPLE_MAX_LENGTH];
    int32_t value_shift;
};

// what a launch names and a plan's header holds: words 1 .. 5 of the header
struct NtupleKey {
    uint32_t n, tuples, shift, n_weights, hash;
};

// NULL, or what is wrong with the parameters
inline const char* ntuple_check(int n, const NtupleParams* p) {
    if (n < 4 || n > 16) return "board_size must be in [4, 16]";
    if (p->tuples < 1 || p->tuples > NTUPLE_MAX_TUPLES) return "tuples must be in [1, 32]";
    if (p->value_shift < 0 || p->value_shift > NTUPLE_MAX_SHIFT) return "value_shift must be in [0, 24]";
    for (int t = 0; t < p->tuples; ++t) {
        if (p->length[t] < 1 || p->length[t] > NTUPLE_MAX_LENGTH) return "a tuple's length must be in [1, 8]";
        for (int i = 0; i < p->length[t]; ++i) {
            if (p->squares[t][i] < 0 || p->squares[t][i] >= n * n) return "a tuple's squares must be in [0, N*N)";
            for (int j = 0; j < i; ++j)
                if (p->squares[t][j] == p->squares[t][i]) return "a tuple's squares must be distinct";
        }
    }
    return nullptr;
}

inline uint32_t ntuple_pow3(int l) {
    uint32_t p = 1;
    for (int i = 0; i < l; ++i) p *= 3u;
    return p;
}

// n_weights = sum_t 3^length[t] (checked parameters: at most 32 * 6561)
inline uint32_t ntuple_n_weights(const NtupleParams& p) {
    uint32_t s = 0;
    for (int t = 0; t < p.tuples; ++t) s += ntuple_pow3(p.length[t]);
    return s;
}

inline uint64_t ntuple_plan_bytes(const NtupleParams& p) { return 4ull * (NTUPLE_HEAD + NTUPLE_REC * (uint64_t)p.tuples); }

// sigma_s(a) of the header's comment on oth_replay_gather
inline int ntuple_sigma(int n, int s, int a) {
    const int r = a / n, c = a % n;
    const int r1 = (s & 1) ? c : r, c1 = (s & 1) ? r : c;
    const int r2 = (s & 2) ? n - 1 - r1 : r1, c2 = (s & 4) ? n - 1 - c1 : c1;
    return r2 * n + c2;
}

// FNV-1a over the lengths and squares that are read
inline uint32_t ntuple_hash(const NtupleParams& p) {
    uint32_t h = 2166136261u;
    for (int t = 0; t < p.tuples; ++t) {
        h = (h ^ (uint32_t)p.length[t]) * 16777619u;
        for (int i = 0; i < p.length[t]; ++i) h = (h ^ (uint32_t)p.squares[t][i]) * 16777619u;
    }
    return h;
}

inline NtupleKey ntuple_key(int n, const NtupleParams& p) {
    return NtupleKey{(uint32_t)n, (uint32_t)p.tuples, (uint32_t)p.value_shift, ntuple_n_weights(p), ntuple_hash(p)};
}

// the plan of checked parameters: ntuple_plan_bytes(p) / 4 words
inline void ntuple_plan(int n, const NtupleParams& p, uint32_t* out) {
    const NtupleKey k = ntuple_key(n, p);
    out[0] = NTUPLE_TAG;
    out[1] = k.n;
    out[2] = k.tuples;
    out[3] = k.shift;
    out[4] = k.n_weights;
    out[5] = k.hash;
    out[6] = (uint32_t)(NTUPLE_HEAD + NTUPLE_REC * p.tuples);
    out[7] = 0u;
    uint32_t off = 0;
    for (int t = 0; t < p.tuples; ++t) {
        uint32_t* rec = out + NTUPLE_HEAD + NTUPLE_REC * t;
        rec[0] = off;
        rec[1] = (uint32_t)p.length[t];
        off += ntuple_pow3(p.length[t]);
        for (int s = 0; s < 8; ++s) {
            uint32_t w[2] = {0u, 0u};
            for (int i = 0; i < p.length[t]; ++i) w[i >> 2] |= (uint32_t)ntuple_sigma(n, s, p.squares[t][i]) << 8 * (i & 3);
            rec[2 + 2 * s] = w[0];
            rec[3 + 2 * s] = w[1];
        }
    }
}

// the plan is the one of these parameters (a block- and call-uniform test)
OTH_HD bool ntuple_plan_is(const uint32_t* plan, const NtupleKey& k) {
    return plan[0] == NTUPLE_TAG && plan[1] == k.n && plan[2] == k.tuples && plan[3] == k.shift &&
           plan[4] == k.n_weights && plan[5] == k.hash && plan[6] == NTUPLE_HEAD + NTUPLE_REC * k.tuples;
}

// c(a): 1 for the mover's disc, 2 for the opponent's, 0 for neither; the mover wins on a square set in both
OTH_HD uint32_t ntuple_cell(const uint64_t* M, const uint64_t* O, uint32_t a) {
    const uint32_t m = (uint32_t)(M[a >> 6] >> (a & 63u)) & 1u, o = (uint32_t)(O[a >> 6] >> (a & 63u)) & 1u;
    return m | (o & ~m) << 1;
}

// off_t + idx_{t,s}: the entry tuple record `rec` hits under symmetry s
OTH_HD uint32_t ntuple_entry(const uint32_t* rec, int s, const uint64_t* M, const uint64_t* O) {
    const uint32_t len = rec[1] < 8u ? rec[1] : 8u, lo = rec[2 + 2 * s], hi = rec[3 + 2 * s];
    uint32_t idx = 0, p = 1;
    for (uint32_t i = 0; i < len; ++i) {
        const uint32_t a = ((i < 4 ? lo : hi) >> 8 * (i & 3u)) & 255u;
        idx += p * ntuple_cell(M, O, a);
        p *= 3u;
    }
    return rec[0] + idx;
}

// symmetry s's share of the sum: sum_t w[off_t + idx_{t,s}]
OTH_HD int64_t ntuple_sum_sym(const uint32_t* plan, int tuples, int s, const int32_t* w, const uint64_t* M,
                              const uint64_t* O) {
    int64_t acc = 0;
    for (int t = 0; t < tuples; ++t) {
        const uint32_t e = ntuple_entry(plan + NTUPLE_HEAD + NTUPLE_REC * t, s, M, O);
        acc += e < plan[4] ? (int64_t)w[e] : 0;  // (always inside, for a plan of these parameters)
    }
    return acc;
}

// S = bias + sum_t sum_s w[off_t + idx_{t,s}]
OTH_HD int64_t ntuple_sum(const uint32_t* plan, const int32_t* w, const uint64_t* M, const uint64_t* O) {
    const int tuples = (int)plan[2];
    int64_t acc = (int64_t)w[plan[4]];
    for (int s = 0; s < 8; ++s) acc += ntuple_sum_sym(plan, tuples, s, w, M, O);
    return acc;
}

OTH_HD int32_t ntuple_value(int64_t sum, int shift) {
    const int64_t v = sum >> shift;
    return (int32_t)(v < -NTUPLE_VALUE_ONE ? -NTUPLE_VALUE_ONE : (v > NTUPLE_VALUE_ONE ? NTUPLE_VALUE_ONE : v));
}

// d = clamp(((clamp(target) - value) rate) rounded to nearest at rate_shift, -2^30, 2^30)
OTH_HD int32_t ntuple_delta(int32_t target, int32_t value, int32_t rate, int rate_shift) {
    const int64_t t = target < -NTUPLE_VALUE_ONE ? -NTUPLE_VALUE_ONE : (target > NTUPLE_VALUE_ONE ? NTUPLE_VALUE_ONE : target);
    int64_t x = (t - (int64_t)value) * (int64_t)rate;
    if (rate_shift >= 1) x = (x + ((int64_t)1 << (rate_shift - 1))) >> rate_shift;
    return (int32_t)(x < -NTUPLE_DELTA_MAX ? -NTUPLE_DELTA_MAX : (x > NTUPLE_DELTA_MAX ? NTUPLE_DELTA_MAX : x));
}

// the mover's and the opponent's words of a row in the exchange format
template <int W>
OTH_HD void ntuple_row(const uint64_t* boards, const uint16_t* meta, size_t r, uint64_t* M, uint64_t* O) {
    const bool tw = (meta[r] & 1u) != 0;
    for (int k = 0; k < W; ++k) {
        const uint64_t b = boards[r * 2 * W + k], wt = boards[r * 2 * W + W + k];
        M[k] = tw ? wt : b;
        O[k] = tw ? b : wt;
    }
}

// One row on the host: value and sum (sums may be NULL)
template <int W>
inline void ntuple_eval_row_host(const uint32_t* plan, const int32_t* w, const uint64_t* boards, const uint16_t* meta,
                                 size_t r, int32_t* values, int64_t* sums) {
    uint64_t M[W], O[W];
    ntuple_row<W>(boards, meta, r, M, O);
    const int64_t S = ntuple_sum(plan, w, M, O);
    values[r] = ntuple_value(S, (int)plan[3]);
    if (sums) sums[r] = S;
}

// One row's additions on the host (the device's are atomics on the same words): d once per hit and
// once on the bias, modulo 2^32
template <int W>
inline void ntuple_add_row_host(const uint32_t* plan, uint32_t* w, const uint64_t* boards, const uint16_t* meta, size_t r,
                                int32_t d) {
    uint64_t M[W], O[W];
    ntuple_row<W>(boards, meta, r, M, O);
    const int tuples = (int)plan[2];
    for (int s = 0; s < 8; ++s)
        for (int t = 0; t < tuples; ++t) w[ntuple_entry(plan + NTUPLE_HEAD + NTUPLE_REC * t, s, M, O)] += (uint32_t)d;
    w[plan[4]] += (uint32_t)d;
}

// The search's evaluation: the plan (LDS on the device), the weights and the game end's weight
struct NtupleEval {
    const uint32_t* plan;
    const int32_t* weights;
    int terminal;
};

// the frontier's H(M, O): the n-tuple value from M's side
template <int N>
OTH_HD int ntuple_leaf(const BB<Geo<N>::W>& M, const BB<Geo<N>::W>& O, const NtupleEval& ev) {
    return ntuple_value(ntuple_sum(ev.plan, ev.weights, M.w, O.w), (int)ev.plan[3]);
}

// One node step of a live task: search_step with the n-tuple value as rule 2.  The other side's
// scan is the game-end test's alone.  The child is On to move against Mn, and H is taken from the
// side to move there: the node's mover gets -H(On, Mn).
template <int N>
OTH_HD void ntuple_search_step(RootTask<N>& s, uint32_t* st, uint32_t max_nodes, int depth, const NtupleEval& ev) {
    constexpr int W = Geo<N>::W;
    if (node_backup<N, SearchFrame<N>>(s, st)) return;
    BB<W> Mn, On;
    if (!node_place<N>(s, max_nodes, Mn, On)) return;
    const bool frontier = s.sp + 1 >= depth;  // the child has no disc left to place
    const BB<W> Lc = solve_legal<N>(On, Mn);
    BB<W> Lo = zero<W>();
    if (!any(Lc)) Lo = solve_legal<N>(Mn, On);
    int v;  // a leaf's value, from this node's mover's side
    if (!any(Lc) && !any(Lo)) {
        v = ev.terminal * (popcount(Mn) - popcount(On));
    } else if (frontier) {
        v = -ntuple_leaf<N>(On, Mn, ev);
    } else {
        // (never: depth <= SEARCH_MAX_DEPTH; kept for memory safety)
        if (s.sp >= SEARCH_MAX_DEPTH - 1) return task_abandon<N>(s);
        const bool passed = !any(Lc);
        return node_descend<N, SearchFrame<N>>(s, st, Mn, On, passed ? Lo : Lc, passed);
    }
    s.best = s.best > v ? s.best : v;
}

// One board on the host (the tests' host build)
template <int N>
inline int ntuple_search_board_host(const uint64_t* black, const uint64_t* white, const uint64_t* stored, uint32_t meta,
                                    int depth, const uint32_t* plan, const int32_t* weights, int terminal,
                                    uint32_t max_nodes, int32_t* value, int32_t* best, int32_t* move_values,
                                    uint64_t* nodes) {
    using Board = BB<Geo<N>::W>;
    const NtupleEval ev{plan, weights, terminal};
    return root_moves_host<N, SearchFrame<N>>(
        black, white, stored, meta,
        [&](const Board& B, const Board& Wt, const Board& Lg, uint32_t m, int& v) {
            return search_status<N>(B, Wt, Lg, m, terminal, v);
        },
        [&](RootTask<N>& s, uint32_t* st) { ntuple_search_step<N>(s, st, max_nodes, depth, ev); }, value, best,
        move_values, nodes);
}

}  // namespace oth
