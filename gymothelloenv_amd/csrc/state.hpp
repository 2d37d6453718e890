// state.hpp -- a board on the device: the meta word's bits, the reset position
// (Start, start_moves, start_fills), the per-lane state (Lane, load / store,
// reset_lane and its pieces), a launch's draw context (Rng) and the W/D/L tallies
// (tally per block, WaveSlot per wave).
//
// One board per lane.  A board is two W-word bitboards (black, white) held in
// VGPRs; legal moves and flips are Kogge-Stone occluded fills (bitboard.hpp).
// HBM layout (exchange format, see the header): boards [E][2W] u64 (a lane
// reads 16W contiguous bytes: dwordx4 loads), meta [E] u16, legal [E][W] u64;
// per-ply outputs are [ply][E] so every store instruction is coalesced.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "bitboard.hpp"
#include "othello_mi355x.h"
#include "tables.hpp"

using namespace oth;

#ifndef OTH_BLOCK
#define OTH_BLOCK 256
#endif

namespace oth_dev {

constexpr int BLOCK = OTH_BLOCK;
constexpr uint32_t M_TURN_WHITE = 1u;
constexpr uint32_t M_TERMINATED = 2u;
constexpr int M_WINNER_SHIFT = 2;
constexpr int M_RAND_SHIFT = 8;
constexpr int BLACK_DISK = -1, NO_DISK = 0, WHITE_DISK = 1;  // othello.py:10-12

// Philox "purpose" word: which decision a draw feeds.
constexpr uint32_t RNG_ACTION = 0, RNG_OPENING_AUTO = 1, RNG_OPENING_RESET = 2;
constexpr uint32_t RNG_PUCT_PICK = 4;  // oth_puct_pick's sampled move (3 is the sampler's, masked.hpp RNG_SAMPLE)
constexpr uint32_t RNG_REPLAY_SAMPLE = 5;  // oth_replay_sample's row and symmetry (replay.hpp)
constexpr uint32_t RNG_PUCT_NOISE = 6;  // oth_puct_noise's table draws (noise.hpp); bits 8 .. 15 hold the block of squares
constexpr uint32_t RNG_NET_MOVE = 7;  // the network's sampled move (play_net.hpp: oth_play_net and the vs calls)
constexpr uint32_t RNG_NTUPLE_EXPLORE = 8;  // the n-tuple player's exploring ply (play_ntuple.hpp: oth_play_ntuple and the vs calls)

template <int N>
struct Start {  // _reset_board (othello.py:256-263): W at (c-1,c-1),(c,c); B at (c,c-1),(c-1,c)
    static constexpr int W = Geo<N>::W;
    static constexpr int C = N / 2;
    static constexpr BB<W> make(int a0, int a1) {
        BB<W> b{};
        for (int i = 0; i < W; ++i) b.w[i] = 0;
        b.w[a0 / 64] |= 1ull << (a0 % 64);
        b.w[a1 / 64] |= 1ull << (a1 % 64);
        return b;
    }
    static constexpr BB<W> BLACK = make(C * N + (C - 1), (C - 1) * N + C);
    static constexpr BB<W> WHITE = make((C - 1) * N + (C - 1), C * N + C);
};

// black's possible_moves on the reset board (_reset_board + get_possible_actions,
// othello.py:256-263, 313-343), by a compile-time ray walk
template <int N>
constexpr uint64_t start_moves() {
    static_assert(Geo<N>::W == 1, "one-word boards");
    const uint64_t B = Start<N>::BLACK.w[0], Wt = Start<N>::WHITE.w[0];
    uint64_t L = 0;
    for (int a = 0; a < N * N; ++a) {
        if (((B | Wt) >> a) & 1ull) continue;
        for (int dr = -1; dr <= 1; ++dr)
            for (int dc = -1; dc <= 1; ++dc) {
                if (!dr && !dc) continue;
                int r = a / N + dr, c = a % N + dc, run = 0;
                while (r >= 0 && r < N && c >= 0 && c < N && ((Wt >> (r * N + c)) & 1ull)) {
                    r += dr;
                    c += dc;
                    ++run;
                }
                if (run > 0 && r >= 0 && r < N && c >= 0 && c < N && ((B >> (r * N + c)) & 1ull)) L |= 1ull << a;
            }
    }
    return L;
}

// the Fills engine's eight fills on the reset board, black to move (what
// OneWord::legal stores in t for the start position), by the same ray walk:
// t[d] = opponent discs from which going along ray direction d (E, S, SE, SW,
// W, N, NW, NE) through opponent discs -- of the inner columns, except on the
// vertical axis, as the scan's propagators -- ends on an own disc
template <int N>
struct StartFills {
    uint64_t t[8];
};
template <int N>
constexpr StartFills<N> start_fills() {
    static_assert(Geo<N>::W == 1, "one-word boards");
    const uint64_t P = Start<N>::BLACK.w[0], O = Start<N>::WHITE.w[0], IN = Geo<N>::INNER.w[0];
    constexpr int DR[8] = {0, 1, 1, 1, 0, -1, -1, -1}, DC[8] = {1, 0, 1, -1, -1, 0, -1, 1};
    StartFills<N> f{};
    for (int d = 0; d < 8; ++d) {
        const uint64_t p1 = DC[d] == 0 ? O : (O & IN);
        f.t[d] = 0;
        for (int a = 0; a < N * N; ++a) {
            if (!((p1 >> a) & 1ull)) continue;
            int r = a / N + DR[d], c = a % N + DC[d];
            while (r >= 0 && r < N && c >= 0 && c < N && ((p1 >> (r * N + c)) & 1ull)) {
                r += DR[d];
                c += DC[d];
            }
            if (r >= 0 && r < N && c >= 0 && c < N && ((P >> (r * N + c)) & 1ull)) f.t[d] |= 1ull << a;
        }
    }
    return f;
}

template <int N>
struct Lane {
    static constexpr int W = Geo<N>::W;
    BB<W> black, white, legal;
    uint32_t meta;
};

template <int N>
__device__ __forceinline__ void load_lane(Lane<N>& s, const uint64_t* __restrict__ boards,
                                          const uint16_t* __restrict__ meta, const uint64_t* __restrict__ legal,
                                          int e) {
    constexpr int W = Geo<N>::W;
    const ulonglong2* bp = reinterpret_cast<const ulonglong2*>(boards) + (size_t)e * W;
    uint64_t tmp[2 * W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
        ulonglong2 v = bp[i];
        tmp[2 * i] = v.x;
        tmp[2 * i + 1] = v.y;
    }
#pragma unroll
    for (int i = 0; i < W; ++i) {
        s.black.w[i] = tmp[i];
        s.white.w[i] = tmp[W + i];
        s.legal.w[i] = legal[(size_t)e * W + i];
    }
    s.meta = meta[e];
}

template <int N>
__device__ __forceinline__ void store_lane(const Lane<N>& s, uint64_t* __restrict__ boards,
                                           uint16_t* __restrict__ meta, uint64_t* __restrict__ legal, int e) {
    constexpr int W = Geo<N>::W;
    uint64_t tmp[2 * W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
        tmp[i] = s.black.w[i];
        tmp[W + i] = s.white.w[i];
    }
    ulonglong2* bp = reinterpret_cast<ulonglong2*>(boards) + (size_t)e * W;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        ulonglong2 v;
        v.x = tmp[2 * i];
        v.y = tmp[2 * i + 1];
        bp[i] = v;
        legal[(size_t)e * W + i] = s.legal.w[i];
    }
    meta[e] = (uint16_t)s.meta;
}

// The meta word of a reset board: black to move, live, and rand_left =
// SimpleOthelloEnv's random-opening length randint(0, k//2+1)*2
// (othello.py:62-63) from Philox.
__device__ __forceinline__ uint32_t reset_meta(uint64_t seed, uint32_t id, uint64_t ply, uint32_t purpose,
                                               int init_rand) {
    uint32_t rl = 0;
    if (init_rand > 0) rl = (uint32_t)scale_index(opening_draw(seed, id, ply, purpose), init_rand / 2 + 1) * 2u;
    return (rl & 0xffu) << M_RAND_SHIFT;
}

// OthelloBaseEnv.reset (othello.py:265-271)
template <int N>
__device__ __forceinline__ void reset_lane(Lane<N>& s, uint64_t seed, uint32_t id, uint64_t ply, uint32_t purpose,
                                           int init_rand) {
    s.black = Start<N>::BLACK;
    s.white = Start<N>::WHITE;
    s.legal = legal_moves<N>(s.black, s.white);  // black moves first (othello.py:267)
    s.meta = reset_meta(seed, id, ply, purpose, init_rand);
}

// The reset position of a one-word board held as words: black to move from
// (B, Wt) with possible_moves L (_reset_board + get_possible_actions,
// othello.py:256-263, 313-343, as compile-time constants), and the Fills engine's
// eight fills of that position, for where they are carried
template <int N>
__device__ __forceinline__ void start_position(uint64_t& B, uint64_t& Wt, uint64_t& L) {
    constexpr uint64_t START_MOVES = start_moves<N>();  // constant-evaluated
    B = Start<N>::BLACK.w[0];
    Wt = Start<N>::WHITE.w[0];
    L = START_MOVES;
}
template <int N>
__device__ __forceinline__ void start_position_fills(uint64_t (&t)[8]) {
    constexpr StartFills<N> SF = start_fills<N>();
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = SF.t[k];
}

// {black wins, draws, white wins} += a finished game's winner
__device__ __forceinline__ void count_winner(int win, uint32_t& cb, uint32_t& cd, uint32_t& cw) {
    cb += win == BLACK_DISK;
    cd += win == NO_DISK;
    cw += win == WHITE_DISK;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Add this block's finished games {black wins, draws, white wins} to its own
// slot wdl[blockIdx.x][0..2].  One slot per block: no atomics, no contention
// (launches on a stream are ordered, and block b of every launch owns slot b);
// oth_counts sums the slots.  Every thread of the block must call this.
__device__ __forceinline__ void tally(unsigned long long* wdl, uint32_t b, uint32_t d, uint32_t w) {
    b = wave_sum(b);
    d = wave_sum(d);
    w = wave_sum(w);
    __shared__ uint32_t part[BLOCK / 64][3];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = b;
        part[wave][1] = d;
        part[wave][2] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0 && wdl) {
        uint32_t sb = 0, sd = 0, sw = 0;
#pragma unroll
        for (int i = 0; i < BLOCK / 64; ++i) {
            sb += part[i][0];
            sd += part[i][1];
            sw += part[i][2];
        }
        if (sb | sd | sw) {
            unsigned long long* slot = wdl + 4 * (size_t)blockIdx.x;
            // only this block touches its slot: uncontended atomics without a
            // return value are posted, so the block does not wait for the slot's
            // read (the read-modify-write cost one memory round trip per launch)
            if (sb) atomicAdd(slot + 0, (unsigned long long)sb);
            if (sd) atomicAdd(slot + 1, (unsigned long long)sd);
            if (sw) atomicAdd(slot + 2, (unsigned long long)sw);
        }
    }
}

// A launch's draw context (and the search depth of OTH_POLICY_MAXIMIN_DEEP launches).
struct Rng {
    uint64_t seed;
    uint32_t id_base;
    int init_rand;
    const uint64_t* ply_off;  // device offset of the ply counter: slot 0 (= 0) eagerly, a graph region's slot under capture
    int depth;                // MaxiMinPolicy(depth) for OTH_POLICY_MAXIMIN_DEEP (depth >= 4)
};

// Per-wave W/D/L slot of a single-ply launch: slot w of the handle's
// [nslots][4] array belongs to wave w of the grid (nslots = ceil(4E / 64) covers
// every wave of a grid of up to four lanes per board; a wave past E reads the
// last live wave's slot and never writes).  The wave's counts accumulate in SGPRs over its boards (three
// ballots per group of 64) and lane 0 adds them with plain stores at the end.
// Launches on a stream are ordered, so the read at a launch's start sees every
// earlier launch's adds.
struct WaveSlot {
    unsigned long long* p;
    unsigned long long v0, v1, v2;
    uint32_t nb = 0, nd = 0, nw = 0;
    __device__ __forceinline__ WaveSlot(unsigned long long* wdl, int t, int E) : WaveSlot(wdl, min(t >> 6, (E - 1) >> 6)) {}
    // slot `wave` (the caller's wave index, clamped to its last live wave)
    __device__ __forceinline__ explicit WaveSlot(unsigned long long* wdl, int wave) {
        // wave-uniform: the slot is read by scalar loads into SGPRs (the values
        // live through the whole kernel; written back by lane 0's vector stores)
        const int w = __builtin_amdgcn_readfirstlane(wave);
        p = wdl + 4 * (size_t)w;
        const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(p);
        v0 = a.x;
        v1 = a.y;
        v2 = p[2];
    }
    // {black wins, draws, white wins} of this wave's lanes (0 / 1 each)
    __device__ __forceinline__ void count(bool b, bool d, bool w) {
        nb += (uint32_t)__popcll(__ballot(b));
        nd += (uint32_t)__popcll(__ballot(d));
        nw += (uint32_t)__popcll(__ballot(w));
    }
    __device__ __forceinline__ void flush() const {
        if ((nb | nd | nw) && (threadIdx.x & 63) == 0) {
            ulonglong2 a;
            a.x = v0 + nb;
            a.y = v1 + nd;
            *reinterpret_cast<ulonglong2*>(p) = a;
            p[2] = v2 + nw;
        }
    }
};

}  // namespace oth_dev
