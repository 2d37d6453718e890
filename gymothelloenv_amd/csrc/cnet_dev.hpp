// cnet_dev.hpp -- the convolutional network of cnet.hpp on the matrix cores: the pieces of k_cnet_eval
// (cnet.hip).  A workgroup of four waves carries RB rows (boards) through the whole network in the LDS.
//
// Activations live in the LDS as int8 [row][(N + 2)^2 padded squares][C] with a halo of zeros that is written
// once and never again, so a tap off the board needs no branch.  Two such images: h (the residual stream) and t
// (the inside of a block).  A 3 x 3 conv is 9 C/64 k-steps of v_mfma_i32_16x16x64_i8 per (output tile, square
// tile): the A operand is a lane-linear 1 KiB weight tile of the blob (one 16-byte global load a lane), the B
// operand is 16 squares x 64 channels: lane 16 g + c reads the 16 channel bytes 64 s + 16 g .. of square c at the
// tap's offset as one ds_read_b128.  The C/D map leaves channels 16 T + 4 g + r of square c on that lane: four
// clipped bytes, one ds_write_b32.  The second conv of a block adds h in place: the lane that owns an output
// element is the only one that reads and writes that element of h during that conv.
//
// Work split: wave w owns two output tiles (og = w mod C/32) and every (4 / (C/32))-th square tile, four square
// tiles at a time: 8 accumulator tiles live, a loaded A tile is used for up to four square tiles and a loaded B
// for two output tiles (6 loads per 8 MFMAs with four square tiles, 4 per 4 with two).
//
// Bank pattern: a pitch of C bytes would put squares c and c + 4 (C = 64) or c + 2 (C = 128) of a ds_read_b128
// lane group on the same 16-byte slot of the 256-byte bank row.  The 16-byte chunk q of a padded square p is
// therefore stored at chunk q ^ swz(p): swz(p) = (-(p >> 2)) & 3 for C = 64 and (p >> 1) & 7 for C = 128, which
// is conflict-free for 16 consecutive padded squares that start at a multiple of 16 (the lane groups of
// ds_read_b128 mix g and g + 1 over c = 4 .. 11: MI355X LDS) and at most 2-way where a tap or a board row's
// end shifts the squares against that grid.
#pragma once
#include <hip/hip_runtime.h>

#include "cnet.hpp"
#include "net_dev.hpp"

namespace oth_dev {

using namespace oth;

constexpr int CNET_THREADS = 256, CNET_WAVES = 4, CNET_SQ = 4;  // square tiles a wave keeps live
enum { CNET_STEM = 0, CNET_FIRST = 1, CNET_SECOND = 2 };

template <int C>
__device__ __forceinline__ int cnet_swz(int p) {
    return C == 64 ? ((-(p >> 2)) & 3) : ((p >> 1) & 7);
}
// the byte of chunk q (16 channels) of padded square p of the block's row rb
template <int C>
__device__ __forceinline__ int cnet_at(const CnetGeo& geo, int rb, int p, int q) {
    return (rb * geo.P2 + p) * C + 16 * (q ^ cnet_swz<C>(p));
}

// rows (boards) a workgroup carries: so that it has about four square tiles
__host__ __device__ inline int cnet_rows_per_block(int ST) { return ST >= 3 ? 1 : (ST == 2 ? 2 : 4); }
// the LDS of a workgroup: h, t, the three input planes as bytes, the logits and the value sums
__host__ __device__ inline size_t cnet_lds_bytes(const CnetGeo& geo, int RB) {
    return 2u * (size_t)RB * geo.P2 * geo.C + (((size_t)RB * 3u * geo.P2 + 15u) & ~(size_t)15u) +
           (((size_t)RB * geo.nn * 4u + 15u) & ~(size_t)15u) + 16u;
}

// the square tile q of the workgroup on this lane: its row, its padded square, whether it is a square at all
struct CnetSq {
    int rb, p;
    bool ok;
};
__device__ __forceinline__ CnetSq cnet_square(const CnetGeo& geo, int q, int c) {
    CnetSq s;
    s.rb = q / geo.ST;
    const int a = 16 * (q - s.rb * geo.ST) + c;
    s.ok = a < geo.nn;
    const int aa = s.ok ? a : geo.nn - 1;  // a padding lane reads a real square; its column of D is never stored
    const int y = aa / geo.n;
    s.p = (y + 1) * geo.NP + (aa - y * geo.n) + 1;
    return s;
}

// One conv over the workgroup's QT square tiles.  part: the conv's biases, then its tiles.  src, dst: the images
// (STEM: src is not read, pl holds the planes' bytes [row][3][P2]).  Every lane executes every MFMA.
template <int C, int MODE>
__device__ __forceinline__ void cnet_conv(const CnetGeo& geo, const uint8_t* __restrict__ part, int shift,
                                          const uint8_t* src, uint8_t* dst, const uint8_t* pl, int QT, int wave,
                                          int lane) {
    constexpr int KS = C / 64, OG = C / 32, SG = CNET_WAVES / OG;
    const int g = lane >> 4, c = lane & 15;
    const int T0 = 2 * (wave % OG), sg = wave / OG;
    const uint8_t* tiles = part + 4 * C;
    for (int q0 = sg; q0 < QT; q0 += CNET_SQ * SG) {
        CnetSq sq[CNET_SQ];
        v4i acc[2][CNET_SQ];
#pragma unroll
        for (int i = 0; i < CNET_SQ; ++i) {
            const int q = q0 + i * SG;
            sq[i] = cnet_square(geo, q < QT ? q : q0, c);
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[t][i] = *reinterpret_cast<const v4i*>(part + 4 * (16 * (T0 + t) + 4 * g));
        }
        if (MODE == CNET_STEM) {
            const v4i a0 = net_tile(tiles, T0, lane), a1 = net_tile(tiles, T0 + 1, lane);
#pragma unroll
            for (int i = 0; i < CNET_SQ; ++i) {
                if (q0 + i * SG < QT) {
                    v4i b = {0, 0, 0, 0};
                    for (int j = 0; j < 16; ++j) {
                        const int k = 16 * g + j;
                        if (k < CNET_STEM_K) {
                            const int pln = k / 9, tap = k - 9 * pln;
                            const int off = (tap / 3 - 1) * geo.NP + (tap % 3 - 1);
                            const int bit = pl[(sq[i].rb * 3 + pln) * geo.P2 + sq[i].p + off];
                            b[j >> 2] |= bit << (8 * (j & 3));
                        }
                    }
                    acc[0][i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b, acc[0][i], 0, 0, 0);
                    acc[1][i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b, acc[1][i], 0, 0, 0);
                }
            }
        } else {
            for (int tap = 0; tap < 9; ++tap) {
                const int off = (tap / 3 - 1) * geo.NP + (tap % 3 - 1);
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const v4i a0 = net_tile(tiles, (T0 * 9 + tap) * KS + s, lane);
                    const v4i a1 = net_tile(tiles, ((T0 + 1) * 9 + tap) * KS + s, lane);
#pragma unroll
                    for (int i = 0; i < CNET_SQ; ++i) {
                        if (q0 + i * SG < QT) {
                            const v4i b =
                                *reinterpret_cast<const v4i*>(src + cnet_at<C>(geo, sq[i].rb, sq[i].p + off, 4 * s + g));
                            acc[0][i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b, acc[0][i], 0, 0, 0);
                            acc[1][i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b, acc[1][i], 0, 0, 0);
                        }
                    }
                }
            }
        }
        // channels 16 T + 4 g + r of this lane's square: four bytes, one store
#pragma unroll
        for (int i = 0; i < CNET_SQ; ++i) {
            if (q0 + i * SG < QT && sq[i].ok) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    uint32_t* at = reinterpret_cast<uint32_t*>(dst + cnet_at<C>(geo, sq[i].rb, sq[i].p, T0 + t) + 4 * g);
                    uint32_t out = 0;
                    if (MODE == CNET_SECOND) {
                        const uint32_t old = *at;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int32_t v = (acc[t][i][r] >> shift) + (int32_t)((old >> (8 * r)) & 255u);
                            out |= (uint32_t)(v < 0 ? 0 : (v > 127 ? 127 : v)) << (8 * r);
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) out |= (uint32_t)net_clip(acc[t][i][r], shift) << (8 * r);
                    }
                    *at = out;
                }
            }
        }
    }
}

// The head: one output tile over the workgroup's square tiles, a tile a wave at a time.  The logit of a square
// goes to zs [row][nn]; the value's terms of the lane's four head outputs are added to vsum[row] (any order of
// an integer sum is exact).
template <int C>
__device__ __forceinline__ void cnet_head(const CnetGeo& geo, const uint8_t* __restrict__ blob, const uint8_t* h,
                                          int32_t* zs, int32_t* vsum, int QT, int wave, int lane) {
    constexpr int KS = C / 64;
    const int g = lane >> 4, c = lane & 15;
    const uint8_t* part = blob + geo.off_head();
    const uint8_t* tiles = part + 64;
    const uint8_t* wv = blob + geo.off_wv();
    for (int q = wave; q < QT; q += CNET_WAVES) {
        const CnetSq sq = cnet_square(geo, q, c);
        v4i u = *reinterpret_cast<const v4i*>(part + 16 * g);
        for (int tap = 0; tap < 9; ++tap) {
            const int off = (tap / 3 - 1) * geo.NP + (tap % 3 - 1);
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const v4i b = *reinterpret_cast<const v4i*>(h + cnet_at<C>(geo, sq.rb, sq.p + off, 4 * s + g));
                u = __builtin_amdgcn_mfma_i32_16x16x64_i8(net_tile(tiles, tap * KS + s, lane), b, u, 0, 0, 0);
            }
        }
        if (sq.ok) {
            const int a = 16 * (q - sq.rb * geo.ST) + c;
            if (g == 0) zs[sq.rb * geo.nn + a] = u[0];
            const uint32_t w4 = *reinterpret_cast<const uint32_t*>(wv + 16 * a + 4 * g);
            int32_t part_sum = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r)  // (head output 0 has a zero byte in wv)
                part_sum += (int32_t)(int8_t)(w4 >> (8 * r)) * (4 * g + r ? net_clip(u[r], geo.shift_head) : 0);
            atomicAdd(&vsum[sq.rb], part_sum);
        }
    }
}

__device__ __forceinline__ int32_t cnet_wave_max(int32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ uint64_t cnet_wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d);
    return v;
}

}  // namespace oth_dev
