// engines.hpp -- the rule engines (who computes legal moves and flips for a lane:
// Solo / Fills / FillsW / Quartet, with the ray tables and RayMath) and
// OthelloBaseEnv.step on a Lane through them (finish_step, step_lane), with the
// random and greedy picks.
#pragma once
#include "state.hpp"

namespace oth_dev {

// ---------------------------------------------------------------------------
// Engines: who computes legal moves and flips for a lane.
//   Solo<N>: one lane per board, all 8 directions (any N).
//   Fills<N> / FillsW<N>: flips from the legal scan's fills and rays -- shifted
//            constants on one-word boards, an LDS ray table on multi-word ones.
//   Quartet<N>: four lanes per board (N <= 8): each lane of the quad scans
//            one axis and the parts are or-ed through DPP quad_perm steps.
// ---------------------------------------------------------------------------
template <int N>
struct Solo {
    static constexpr int RAY_WORDS = 0;
    static constexpr bool FLIP_ANY = false;  // flip() is for a square of the board
    __device__ __forceinline__ Solo(int, const uint64_t*) {}
    __device__ __forceinline__ BB<Geo<N>::W> legal(const BB<Geo<N>::W>& P, const BB<Geo<N>::W>& O) const {
        if constexpr (Geo<N>::W == 1) {  // the dword-pair scan (fills unused, so dead)
            uint64_t t[8];
            BB<1> r;
            r.w[0] = OneWord<N>::legal(P.w[0], O.w[0], t);
            return r;
        }
        return legal_moves<N>(P, O);
    }
    __device__ __forceinline__ BB<Geo<N>::W> flip(const BB<Geo<N>::W>& P, const BB<Geo<N>::W>& O, int a) const {
        return flips<N>(P, O, square<Geo<N>::W>(a));
    }
    __device__ __forceinline__ void prime(const Lane<N>&) const {}
    __device__ __forceinline__ bool leader() const { return true; }
};

// Ray tables for one-word boards: rays[d*64 + sq] = the squares strictly beyond
// sq in direction d, up to the edge.  d 0..3 point to higher squares (E, S, SE,
// SW), d 4..7 to lower ones (W, N, NW, NE).  Built in LDS once per launch.
// Steps (row, col) of direction d: RAY_DR = {0, 1, 1, 1, 0, -1, -1, -1},
// RAY_DC = {1, 0, 1, -1, -1, 0, -1, 1} (nibbles of the immediates in fill_rays).

// DIRS: the directions 0 .. DIRS-1 only (the handle's table holds the four up ones, k_fill_rays).
template <int N, int DIRS = 8>
__device__ __forceinline__ void fill_rays(uint64_t* rays) {
    for (int i = threadIdx.x; i < DIRS * 64; i += BLOCK) {
        const int d = i >> 6, sq = i & 63;
        uint64_t r = 0;
        if (sq < N * N) {
            // RAY_DR / RAY_DC as sign-extended nibbles: no constant-memory loads
            const int dr = __builtin_amdgcn_sbfe((int)0xFFF01110u, 4 * d, 4);
            const int dc = __builtin_amdgcn_sbfe((int)0x1F0FF101u, 4 * d, 4);
            int row = sq / N + dr, col = sq % N + dc;
            while (row >= 0 && row < N && col >= 0 && col < N) {
                const int s2 = row * N + col;
                r |= 1ull << s2;
                row += dr;
                col += dc;
            }
        }
        rays[i] = r;
    }
    __syncthreads();
}

// Without a table: the rays of square s toward higher squares (E, S, SE, SW)
// as one shifted constant each -- the ray from square 0 (or row 0's squares
// 1 .. N-1 for E) moved to s -- with the squares that wrapped past the board's
// right (E, SE) or left (SW) edge masked off by column.
template <int N>
struct RayMath {
    static constexpr uint64_t sum_steps(int step, int k0, int k1) {
        uint64_t x = 0;
        for (int k = k0; k <= k1; ++k) x |= 1ull << (k * step);
        return x;
    }
    static constexpr uint64_t BD = Geo<N>::BOARD.w[0];
    static constexpr uint64_t ROW1 = sum_steps(N, 0, N - 1);      // column 0 of every row
    static constexpr uint64_t EAST = ((1ull << N) - 1) & ~1ull;    // squares 1 .. N-1 of row 0
    static constexpr uint64_t COL = sum_steps(N, 1, N - 1);       // S from square 0
    static constexpr uint64_t DIAG = sum_steps(N + 1, 1, N - 1);  // SE from square 0
    static constexpr uint64_t ANTI = sum_steps(N - 1, 1, N - 1);  // SW from square N-1, moved to square 0
    // square s of the board turned by 180 degrees, for any s < 64: an invalid
    // action's square may lie past N*N - 1 on boards of N < 8, so the result is
    // kept below 64 (every shift count of up() stays defined; the caller masks
    // the flips of an invalid action)
    __device__ __forceinline__ static uint32_t turned(uint32_t s) {
        return N == 8 ? N * N - 1 - s : (N * N - 1 - s) & 63u;
    }
    __device__ __forceinline__ static void up(uint32_t s, uint32_t c, uint64_t* ray) {
        const uint32_t row = (1u << N) - 1u;
        const uint64_t gt = ROW1 * (uint64_t)((row << (c + 1)) & row);  // columns > c of every row
        const uint64_t lt = ROW1 * (uint64_t)((1u << c) - 1u);           // columns < c
        ray[0] = (EAST << s) & gt;
        ray[1] = (COL << s) & BD;
        ray[2] = (DIAG << s) & gt & BD;
        ray[3] = (ANTI << s) & lt & BD;
    }
};

// Fills<N>: flips from the legal scan's fills and shifted ray constants (no
// table, no LDS).  legal_moves' axis scans
// compute, for the side to move, the fills t(dir) = opponent discs reachable
// from an own disc through contiguous opponent discs stepping in direction dir
// (the scan shifts them once more onto the empty squares).  Kept in registers
// until the next ply, they answer update_board's capping test: along ray d
// from the played square a, the run to flip is the contiguous part of ray_d(a)
// inside t(-d) -- every square of t(-d) on that run is already capped by an
// own disc further along d.  So per direction: nearest square of the ray NOT
// in t(-d), and the ray squares before it; no test against the own discs.
// The fills are valid for the board they were computed on: every path that
// changes the side to move computes them (legal() in step_lane), and k_play
// primes them after loading or resetting a board.
template <int N>
struct Fills {
    static_assert(Geo<N>::W == 1, "fills engine is for one-word boards (N <= 8)");
    static constexpr int RAY_WORDS = 0;     // no table in LDS
    static constexpr bool FLIP_ANY = true;  // flip() is defined for every a (its shift counts are masked)
    static constexpr int STEPS = Pro<N, 0, 1>::STEPS;
    static constexpr uint64_t BD = Geo<N>::BOARD.w[0], IN = Geo<N>::INNER.w[0];
    // t[d] = the fill to use for ray direction d (rays: E, S, SE, SW, W, N, NW, NE):
    // up directions (+S) use the -S fill, down directions the +S fill
    mutable uint64_t t[8];
    __device__ __forceinline__ Fills(int, const uint64_t*) {}

    // get_possible_actions for mover P, keeping the fills: the axis-paired scan
    // on dwords (bitboard.hpp OneWord: v_bitop3 / v_and_or, carry-chain horizontal axis)
    __device__ __forceinline__ BB<1> legal(const BB<1>& Pb, const BB<1>& Ob) const {
        BB<1> r;
        r.w[0] = OneWord<N>::legal(Pb.w[0], Ob.w[0], t);
        return r;
    }
    // update_board's flips for a move on square a (OneWord::flip_fills: the rays
    // are four constants, held in SGPRs, shifted to a and to the turned square:
    // no LDS round trip behind the pick's sel8 read, for +8 VALU per ply; 8x8
    // random play 67.9 -> 65.1 us per 100-ply launch of 65,536 boards, DESIGN.md
    // section 5).  No column masks as RayMath's rays need (+38 VALU per ply):
    // a fill holds no edge-column square off the vertical axis.
    __device__ __forceinline__ BB<1> flip(const BB<1>&, const BB<1>&, int a) const {
        BB<1> out;
        out.w[0] = OneWord<N>::flip_fills(t, a);
        return out;
    }
    // GreedyPolicy from the fills of the side to move (bitboard.hpp OneWord::greedy)
    __device__ __forceinline__ int greedy(const BB<1>& legal) const { return OneWord<N>::greedy(t, legal.w[0]); }
    // recompute the fills for the side to move (after a load or a reset)
    __device__ __forceinline__ void prime(const Lane<N>& s) const {
        const bool tw = (s.meta & M_TURN_WHITE) != 0;
        (void)legal(pick(tw, s.white, s.black), pick(tw, s.black, s.white));
    }
    __device__ __forceinline__ bool leader() const { return true; }
};

// FillsW<N>: the Fills engine for multi-word boards (N >= 9): the legal scan
// keeps its eight fills (legal_moves_fills) and update_board's flips come from
// them and a ray table of BB<W> entries in LDS (flips_fills), without the
// Kogge-Stone run and capping test per direction.
template <int N>
struct FillsW {
    static constexpr int W = Geo<N>::W;
    static constexpr int RAY_WORDS = 8 * N * N * W;
    static constexpr bool FLIP_ANY = false;  // flip() reads its table at a
    const BB<W>* rays;
    mutable BB<W> t[8];
    __device__ __forceinline__ FillsW(int, const uint64_t* lds) : rays(reinterpret_cast<const BB<W>*>(lds)) {}
    __device__ __forceinline__ BB<W> legal(const BB<W>& P, const BB<W>& O) const {
        return legal_moves_fills<N>(P, O, t);
    }
    __device__ __forceinline__ BB<W> flip(const BB<W>&, const BB<W>&, int a) const {
        return flips_fills<N>(rays, t, a);
    }
    __device__ __forceinline__ void prime(const Lane<N>& s) const {
        const bool tw = (s.meta & M_TURN_WHITE) != 0;
        BB<W> P, O;  // word-wise selects: a select of the two members' addresses puts the lane in scratch
#pragma unroll
        for (int i = 0; i < W; ++i) {
            P.w[i] = tw ? s.white.w[i] : s.black.w[i];
            O.w[i] = tw ? s.black.w[i] : s.white.w[i];
        }
        (void)legal(P, O);
    }
    __device__ __forceinline__ bool leader() const { return true; }
    __device__ static void fill(uint64_t* lds) {
        BB<W>* r = reinterpret_cast<BB<W>*>(lds);
        for (int i = threadIdx.x; i < 8 * N * N; i += BLOCK) r[i] = ray_from<N>(i / (N * N), i % (N * N));
        __syncthreads();
    }
};

template <typename Eng>
struct is_fills_w : std::false_type {};
template <int N>
struct is_fills_w<FillsW<N>> : std::true_type {};


// Quartet<N>: four lanes per board (N <= 8, one word), lanes 4k..4k+3 of a DPP
// quad: lane q scans one axis (E/W, S/N, SE/NW, SW/NE) and computes the flips
// of its two ray directions (q toward higher squares, q + 4 toward lower);
// the four parts are or-ed through quad_perm [1,0,3,2] and [2,3,0,1].  Every
// decision of step_lane is taken on the or-ed (quad-uniform) masks, so the four
// lanes always follow the same branches and the DPP steps never read an
// inactive lane.
template <int N>
struct Quartet {
    static_assert(Geo<N>::W == 1, "Quartet engine is for one-word boards (N <= 8)");
    static constexpr int RAY_WORDS = 8 * 64;
    static constexpr bool FLIP_ANY = true;  // flip() reads its 64-entry tables at any a below 64
    static constexpr uint64_t BD = Geo<N>::BOARD.w[0], IN = Geo<N>::INNER.w[0];
    const uint64_t* rays;  // this lane's "up" table; its "down" table is 4 * 64 words further
    uint32_t sh;           // axis shift: 1, N, N + 1, N - 1
    uint64_t pm;           // propagator mask: the vertical axis may pass edge columns
    int q;
    __device__ __forceinline__ Quartet(int lane_q, const uint64_t* lds) : q(lane_q) {
        rays = lds + 64 * lane_q;
        sh = lane_q == 0 ? 1u : (lane_q == 1 ? (uint32_t)N : (lane_q == 2 ? N + 1u : N - 1u));
        pm = lane_q == 1 ? BD : IN;
    }
    static constexpr int STEPS = Pro<N, 0, 1>::STEPS;
    // legal_moves along one axis (+s and -s) with a per-lane shift amount
    __device__ __forceinline__ static void axis(uint64_t P, uint64_t p1, uint32_t s, uint64_t& L) {
        uint64_t p2 = 0, p4 = 0;
        if constexpr (STEPS > 1) p2 = p1 & (p1 << s);
        if constexpr (STEPS > 2) p4 = p2 & (p2 << (2 * s));
        uint64_t t = (P << s) & p1;
        t |= p1 & (t << s);
        if constexpr (STEPS > 1) t |= p2 & (t << (2 * s));
        if constexpr (STEPS > 2) t |= p4 & (t << (4 * s));
        L |= t << s;
        t = (P >> s) & p1;
        t |= p1 & (t >> s);
        if constexpr (STEPS > 1) t |= (p2 >> s) & (t >> (2 * s));
        if constexpr (STEPS > 2) t |= (p4 >> (3 * s)) & (t >> (4 * s));
        L |= t >> s;
    }
    __device__ __forceinline__ static uint32_t quad_or32(uint32_t x) {
        x |= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, false);
        return x | (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xF, 0xF, false);
    }
    __device__ __forceinline__ static uint64_t quad_or(uint64_t x) {
        return ((uint64_t)quad_or32((uint32_t)(x >> 32)) << 32) | quad_or32((uint32_t)x);
    }
    __device__ __forceinline__ BB<1> legal(const BB<1>& Pb, const BB<1>& Ob) const {
        const uint64_t P = Pb.w[0], O = Ob.w[0];
        uint64_t L = 0;
        axis(P, O & pm, sh, L);
        BB<1> r;
        r.w[0] = quad_or(L) & ~(P | O) & BD;
        return r;
    }
    __device__ __forceinline__ BB<1> flip(const BB<1>& Pb, const BB<1>& Ob, int a) const {
        const uint64_t P = Pb.w[0], nO = ~Ob.w[0];
        uint64_t f;
        {  // toward higher squares: the nearest non-opponent square is the lowest set bit
            const uint64_t ray = rays[a];
            const uint64_t x = ray & nO;
            const uint64_t fb = x & (0ull - x);
            f = (fb & P) ? (ray & (fb - 1ull)) : 0ull;
        }
        {  // toward lower squares: the highest set bit
            const uint64_t ray = rays[4 * 64 + a];
            const uint64_t x = ray & nO;
            const uint64_t hb = x ? (0x8000000000000000ull >> __clzll(x)) : 0ull;
            f |= (hb & P) ? (ray & (0ull - (hb << 1))) : 0ull;
        }
        BB<1> out;
        out.w[0] = quad_or(f);
        return out;
    }
    __device__ __forceinline__ void prime(const Lane<N>&) const {}
};

// The rest of OthelloBaseEnv.step after update_board (othello.py:425-462):
// full board / sudden death, the opponent's legal moves, pass and double pass,
// winner and reward.  P / O are the mover's / opponent's discs after the move.
template <int N, typename Eng>
__device__ __forceinline__ void finish_step(Lane<N>& s, bool tw, bool valid, const BB<Geo<N>::W>& P,
                                            const BB<Geo<N>::W>& O, uint32_t flags, int& reward, int& done,
                                            int& winner, const Eng& eng) {
    constexpr int W = Geo<N>::W;
    constexpr int NN = N * N;
    const bool full = !any(~(P | O) & Geo<N>::BOARD);                       // :425-426
    const bool sudden = !valid && (flags & OTH_SUDDEN_DEATH);              // :427
    const int pc = popcount(P), oc = popcount(O);
    const int cur = tw ? WHITE_DISK : BLACK_DISK;
    const int by_count = pc > oc ? cur : (pc < oc ? -cur : NO_DISK);       // determine_winner (:486-501)
    bool term = false, new_tw = tw;
    if (sudden || full) {  // :431-433 -- turn and possible_moves stay stale
        term = true;
        winner = sudden ? -cur : by_count;  // :475-485
    } else {               // :436-442
        const BB<W> om = eng.legal(O, P);
        const bool opp_pass = !any(om);
        BB<W> nl = om;
        if (opp_pass) nl = eng.legal(P, O);
        s.legal = nl;
        if (!opp_pass) {
            new_tw = !tw;
        } else if (!any(nl)) {  // nobody can move
            term = true;
            winner = by_count;
        }
    }
    s.white = pick(tw, P, O);  // word-wise: a store through a selected member address puts the lane in scratch
    s.black = pick(tw, O, P);
    int r = 0;  // :444-461
    if (term) {
        if (flags & OTH_DISK_REWARD) {
            r = sudden ? -NN : (oc == 0 ? NN : pc - oc);
        } else {
            r = winner * cur;
        }
    }
    const uint32_t wcode = winner == WHITE_DISK ? 1u : (winner == BLACK_DISK ? 2u : 0u);
    s.meta = (s.meta & 0xff00u) | (new_tw ? M_TURN_WHITE : 0u) | (term ? M_TERMINATED : 0u) |
             (term ? (wcode << M_WINNER_SHIFT) : 0u);
    reward = r;
    done = term ? 1 : 0;
}

// OthelloBaseEnv.step (othello.py:412-462) for one lane.  Returns the winner
// code (0 none) through `winner` when the game ends on this ply.
// PICKED: `a` is a policy's pick from s.legal, or -1 when s.legal is empty, so
// validity is a >= 0 and the flip is computed without a branch and masked.
template <int N, typename Eng, bool PICKED = false>
__device__ __forceinline__ void step_lane(Lane<N>& s, int a, uint32_t flags, int& reward, int& done, int& winner,
                                          const Eng& eng) {
    constexpr int W = Geo<N>::W;
    constexpr int NN = N * N;
    winner = NO_DISK;
    if (s.meta & M_TERMINATED) {  // reference: ValueError (othello.py:415-416)
        reward = 0;
        done = 1;
        return;
    }
    const bool tw = (s.meta & M_TURN_WHITE) != 0;
    BB<W> P = pick(tw, s.white, s.black);
    BB<W> O = pick(tw, s.black, s.white);
    if constexpr (PICKED && Eng::FLIP_ANY && W == 1) {
        const bool valid = a >= 0;
        const uint64_t m = valid ? 1ull << (a & 63) : 0ull;
        const uint64_t f = eng.flip(P, O, a & 63).w[0] & (0ull - (uint64_t)valid);
        P.w[0] |= f | m;
        O.w[0] &= ~(f | m);
        finish_step<N>(s, tw, valid, P, O, flags, reward, done, winner, eng);
        return;
    }
    const bool valid = a >= 0 && a < NN && test(s.legal, a);  // `action not in possible_moves` (:417)
    if (valid) {                                               // update_board (:391-410)
        const BB<W> m = square<W>(a);
        const BB<W> f = eng.flip(P, O, a);
        P |= f | m;
        O = O & ~(f | m);
    }
    finish_step<N>(s, tw, valid, P, O, flags, reward, done, winner, eng);
}

// RandomPolicy.get_action (simple_policies.py:37-41): possible_moves[randint(len)]
// with u = the ply's 32-bit draw.
template <int N>
__device__ __forceinline__ int random_action(const Lane<N>& s, uint32_t u) {
    const int n = popcount(s.legal);
    return select_bit(s.legal, scale_index(u, n));
}

// GreedyPolicy.get_action (simple_policies.py:69-92): the move that leaves the
// mover the most discs = the most flips; np.argmax keeps the first (lowest
// square) of equal counts.
template <int N, typename Eng>
__device__ __forceinline__ int greedy_action(const Lane<N>& s, const Eng& eng) {
    // every square's flip count on bit planes, no loop over the candidates
    if constexpr (std::is_same<Eng, Fills<N>>::value) {
        return eng.greedy(s.legal);  // the fills of the side to move are carried from the last scan
    } else if constexpr (Geo<N>::W == 1) {
        const bool tw = (s.meta & M_TURN_WHITE) != 0;
        uint64_t t[8];
        (void)OneWord<N>::legal(tw ? s.white.w[0] : s.black.w[0], tw ? s.black.w[0] : s.white.w[0], t);
        return OneWord<N>::greedy(t, s.legal.w[0]);
    } else if constexpr (is_fills_w<Eng>::value) {  // multi-word boards: the same planes on BB<W> (PlanesW)
        return PlanesW<N>::greedy(eng.t, s.legal);  // fills carried from the last scan
    } else {
        const bool tw = (s.meta & M_TURN_WHITE) != 0;
        BB<Geo<N>::W> t[8];
        (void)legal_moves_fills<N>(pick(tw, s.white, s.black), pick(tw, s.black, s.white), t);
        return PlanesW<N>::greedy(t, s.legal);
    }
}

}  // namespace oth_dev
