// noise.hpp -- oth_puct_noise: Dirichlet root noise mixed into rows of priors, in integers (the
// spec is the header's comment on oth_puct_noise: every output is an integer function of the row,
// the handle's position, epsilon, the table, the seed, the global env id and the counter).
//
// The part outside __HIPCC__ is plain host/device code: whether a board takes noise, one
// square's table draw, and one row (noise_row: two passes over the legal squares, the sum of the
// draws and then the division).  tests/host/noise_host.cpp compiles it with g++ and loops over
// the rows; the device kernel (below, noise.hip's) runs the same text, a lane a board.  N and W
// are run-time values: nothing here needs them at compile time.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>

#include "bitboard.hpp"

namespace oth {

constexpr int NOISE_TABLE = 4096, NOISE_MAX_EPSILON = 256, NOISE_LEAF_EXPAND = 1;
constexpr uint32_t NOISE_G_MAX = 1u << 24;
constexpr uint32_t NOISE_RNG = 6u;  // Philox purpose of the draws (state.hpp RNG_PUCT_NOISE); bits 8 .. 15: the block

// floor(num / den) for num < 2^53, 0 < den < 2^53 (puct_floor_div's way: the double's quotient is
// within one of it, an integer correction makes it exact without a 64-bit division)
OTH_HD uint64_t noise_floor_div(uint64_t num, uint64_t den) {
    uint64_t q = (uint64_t)((double)num / (double)den);
    if (q * den > num) --q;
    else if ((q + 1) * den <= num) ++q;
    return q;
}

// the Philox block of squares 4 b .. 4 b + 3 of a board, and square a's clamped table entry from it
OTH_HD U4 noise_block(uint64_t seed, uint32_t id, uint64_t counter, uint32_t b) {
    return philox4(seed, id, counter, NOISE_RNG | b << 8);
}
OTH_HD uint32_t noise_g(const uint32_t* table, const U4& blk, int a) {
    const uint32_t g = table[pick4(blk, (uint32_t)a & 3u) >> 20];
    return g > NOISE_G_MAX ? NOISE_G_MAX : g;
}

// the handle's stored possible_moves word j, restricted to the board of nn squares
OTH_HD uint64_t noise_moves_word(const uint64_t* stored, int j, int nn) {
    const int left = nn - 64 * j;
    return left >= 64 ? stored[j] : (left <= 0 ? 0ull : stored[j] & ((1ull << left) - 1ull));
}

// leaf mode: the pending leaf of the board's first row is the root itself
OTH_HD bool noise_applies(int W, uint8_t kind, const uint64_t* leaf_board, const uint64_t* handle_board) {
    bool same = kind == (uint8_t)NOISE_LEAF_EXPAND;
    for (int j = 0; j < 2 * W; ++j) same = same && leaf_board[j] == handle_board[j];
    return same;
}

// One applied row: in and out the row's nn priors (they may be the same), stored the handle's
// possible_moves of the board (W words).  Squares outside the moves are copied; with no move or a
// zero sum of draws the whole row is.
OTH_HD void noise_row(int nn, int W, const uint64_t* stored, const int32_t* in, int32_t* out, int32_t epsilon,
                      const uint32_t* table, uint64_t seed, uint32_t id, uint64_t counter) {
    uint64_t G = 0;
    for (int j = 0; j < W; ++j) {
        uint64_t m = noise_moves_word(stored, j, nn);
        uint32_t have = 0xffffffffu;
        U4 blk{0u, 0u, 0u, 0u};
        while (m) {
            const int a = 64 * j + ctz64(m);
            m &= m - 1ull;
            if ((uint32_t)a >> 2 != have) blk = noise_block(seed, id, counter, have = (uint32_t)a >> 2);
            G += noise_g(table, blk, a);
        }
    }
    if (in != out)
        for (int a = 0; a < nn; ++a) out[a] = in[a];
    if (G == 0) return;
    const uint64_t keep = (uint64_t)(NOISE_MAX_EPSILON - epsilon), eps = (uint64_t)epsilon;
    for (int j = 0; j < W; ++j) {
        uint64_t m = noise_moves_word(stored, j, nn);
        uint32_t have = 0xffffffffu;
        U4 blk{0u, 0u, 0u, 0u};
        while (m) {
            const int a = 64 * j + ctz64(m);
            m &= m - 1ull;
            if ((uint32_t)a >> 2 != have) blk = noise_block(seed, id, counter, have = (uint32_t)a >> 2);
            const uint64_t eta = noise_floor_div(65535ull * noise_g(table, blk, a) + G / 2u, G);
            const int32_t p = in[a];
            const uint64_t pc = (uint64_t)(p < 0 ? 0 : (p > 65535 ? 65535 : p));
            out[a] = (int32_t)((keep * pc + eps * eta + 128u) >> 8);
        }
    }
}

// oth_puct_noise for board e of E, K rows a board (kind and boards NULL: root mode)
OTH_HD void noise_board(int nn, int W, int K, size_t e, const uint64_t* handle_boards, const uint64_t* handle_legal,
                        const uint8_t* kind, const uint64_t* boards, const int32_t* in, int32_t* out, int32_t epsilon,
                        const uint32_t* table, uint64_t seed, uint32_t id, uint64_t counter) {
    const size_t r0 = e * (size_t)K;
    const bool apply = !kind || noise_applies(W, kind[r0], boards + r0 * 2 * W, handle_boards + e * 2 * W);
    if (apply)
        noise_row(nn, W, handle_legal + e * W, in + r0 * nn, out + r0 * nn, epsilon, table, seed, id, counter);
    if (in == out) return;
    for (size_t r = apply ? r0 + 1 : r0; r < r0 + (size_t)K; ++r)
        for (int a = 0; a < nn; ++a) out[r * nn + a] = in[r * nn + a];
}

}  // namespace oth
