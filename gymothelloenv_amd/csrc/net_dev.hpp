// net_dev.hpp -- the network of net.hpp on the matrix cores: net_eval_tile, a wave's tile of 16 rows through
// all layers, the head and the integer softmax.  k_net_eval (net.hip: rows from global memory, the results to
// global memory) and k_play_net (play_net.hpp: rows from the LDS, the results read there by the boards' owners)
// are both thin callers: the arithmetic of the network exists once.
//
// A wave carries a tile of 16 rows through all layers on v_mfma_i32_16x16x64_i8.  The weights are the A operand
// (a tile of 16 outputs x 64 inputs, lane-linear in the blob: one 16-byte load a lane), the rows are the B
// operand (64 inputs x 16 rows): lane 16 g + c holds 16 input bytes of row c.  The C/D map puts row c's outputs
// 4 g + r (r = 0 .. 3) of an output tile on that same lane, so the clipped int8 outputs of four output tiles,
// packed into four registers, are that lane's 16 bytes of one k-step of the next layer: no lane movement and no
// LDS between layers; the next layer's k order (net_kh) is permuted in the packed weights instead.  The first
// layer's operand is made in registers from the bit words: 16 bits become 16 bytes.
//
// The head's logits of a row lie on four lanes (g = 0 .. 3); they wait in the LDS (each lane reads back only what
// it wrote) between the pass that finds the row's largest legal logit, the pass that sums the e_a, and the pass
// that divides; the maximum and the sum cross the four lanes by two shuffles.
#pragma once
#include <hip/hip_runtime.h>

#include "net.hpp"

namespace oth_dev {

using namespace oth;

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int NET_ROWS = 16;  // rows a wave

// tools/probe_net.py's variants, never the shipped library: 1, 2, 3 end the evaluation after layer 0, after the
// hidden layers, after the head's logits (one word of what was computed is handed back, so that it is computed)
#ifndef OTH_NET_STOP
#define OTH_NET_STOP 0
#endif

__device__ __forceinline__ v4i net_tile(const uint8_t* __restrict__ tiles, int tile, int lane) {
    return *reinterpret_cast<const v4i*>(tiles + ((size_t)tile * 64 + (size_t)lane) * 16);
}

// 16 bits to 16 bytes of 0 or 1: a nibble times (1 + 2^7 + 2^14 + 2^21) has bit b of it at bit 8 b
__device__ __forceinline__ v4i net_spread(uint32_t bits) {
    v4i r;
#pragma unroll
    for (int t = 0; t < 4; ++t) r[t] = (int)((((bits >> (4 * t)) & 15u) * 0x00204081u) & 0x01010101u);
    return r;
}

// four output tiles to the next layer's 16 bytes: byte 4 t + r is output 4 g + r of tile t
__device__ __forceinline__ v4i net_acts(const v4i* acc, int shift) {
    v4i r;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        r[t] = net_clip(acc[t][0], shift) | net_clip(acc[t][1], shift) << 8 | net_clip(acc[t][2], shift) << 16 |
               net_clip(acc[t][3], shift) << 24;
    return r;
}

// where output o = 16 T + 4 g + r of row c waits in zs (int32 [OT][4][64]): lane 16 g + c's own word
__device__ __forceinline__ int net_zs_index(int o, int c) { return (4 * (o >> 4) + (o & 3)) * 64 + 4 * (o & 12) + c; }

// what an evaluation hands back beside zs: whether the row has a legal square (the same on the row's four lanes)
// and, in the OTH_NET_STOP variants, the word that keeps the cut-short computation alive
struct NetTileOut {
    bool any;
    int32_t stop;
};

// One tile: the lane 16 g + c carries row c.  words(p, v): word v of plane p (0 the mover's discs, 1 the
// opponent's, 2 the legal squares) of this lane's row, 0 for a row that is not live; head(o, z): called once for
// each of this lane's head outputs o = 16 T + 4 g + r (o < 16 OT: the logits o < nn, the value's z at o = nn,
// padding behind it) with its accumulator.  Leaves in zs, at net_zs_index(a, c), the prior of square a < nn of row
// c (0 on a row without a legal square): written by the row's own lanes, so another lane reads it after a
// barrier.  Every lane of the wave executes every MFMA.
template <int KS, class Words, class Head>
__device__ __forceinline__ NetTileOut net_eval_tile(const NetGeo& geo, const uint8_t* __restrict__ blob,
                                                    int32_t* __restrict__ zs, int lane, Words words, Head head) {
    const int g = lane >> 4;
    const int W = geo.W, nn = geo.nn;
    NetTileOut out{false, 0};

    // layer 0: every output tile's accumulator live, a k-step a word of a plane
    v4i acc[4 * KS];
    {
        const uint8_t* bias = blob + geo.off_bias(0);
        const uint8_t* tiles = blob + geo.off_tiles(0);
#pragma unroll
        for (int T = 0; T < 4 * KS; ++T) acc[T] = *reinterpret_cast<const v4i*>(bias + 64 * T + 16 * g);
        for (int s = 0; s < geo.K0S; ++s) {
            const int p = s / W, v = s - p * W;
            const uint64_t word = words(p, v);
            const v4i b = net_spread((uint32_t)(word >> (16 * g)) & 0xffffu);
#pragma unroll
            for (int T = 0; T < 4 * KS; ++T)
                acc[T] = __builtin_amdgcn_mfma_i32_16x16x64_i8(net_tile(tiles, T * geo.K0S + s, lane), b, acc[T], 0, 0, 0);
        }
    }
    v4i h[KS];
#pragma unroll
    for (int q = 0; q < KS; ++q) h[q] = net_acts(acc + 4 * q, geo.shift(0));

    if (OTH_NET_STOP == 1) {
#pragma unroll
        for (int q = 0; q < KS; ++q) out.stop ^= h[q][0] ^ h[q][1] ^ h[q][2] ^ h[q][3];
        return out;
    }

    // layers 1 .. L - 1: four output tiles at a time
    for (int l = 1; l < geo.L; ++l) {
        const uint8_t* bias = blob + geo.off_bias(l);
        const uint8_t* tiles = blob + geo.off_tiles(l);
        v4i hn[KS];
#pragma unroll
        for (int q = 0; q < KS; ++q) {
            v4i a4[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) a4[t] = *reinterpret_cast<const v4i*>(bias + 64 * (4 * q + t) + 16 * g);
#pragma unroll
            for (int s = 0; s < KS; ++s)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    a4[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(net_tile(tiles, (4 * q + t) * KS + s, lane), h[s], a4[t],
                                                                  0, 0, 0);
            hn[q] = net_acts(a4, geo.shift(l));
        }
#pragma unroll
        for (int q = 0; q < KS; ++q) h[q] = hn[q];
    }

    if (OTH_NET_STOP == 2) {
#pragma unroll
        for (int q = 0; q < KS; ++q) out.stop ^= h[q][0] ^ h[q][1] ^ h[q][2] ^ h[q][3];
        return out;
    }

    // the head: logit o = 16 T + 4 g + r of row c, kept in the LDS; the largest legal logit
    const uint8_t* bias = blob + geo.off_bias(geo.L);
    const uint8_t* tiles = blob + geo.off_tiles(geo.L);
    int32_t m = INT32_MIN;
    bool any = false;
    for (int T = 0; T < geo.OT; ++T) {
        v4i z = *reinterpret_cast<const v4i*>(bias + 64 * T + 16 * g);
#pragma unroll
        for (int s = 0; s < KS; ++s)
            z = __builtin_amdgcn_mfma_i32_16x16x64_i8(net_tile(tiles, T * KS + s, lane), h[s], z, 0, 0, 0);
        const int o0 = 16 * T + 4 * g;
        const uint64_t lw = (T >> 2) < W ? words(2, T >> 2) : 0ull;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = o0 + r;
            zs[(4 * T + r) * 64 + lane] = z[r];
            head(o, z[r]);
            if (o < nn && ((lw >> (o & 63)) & 1u)) {
                any = true;
                m = z[r] > m ? z[r] : m;
            }
        }
    }
    if (OTH_NET_STOP == 3) {
        out.stop = m;
        return out;
    }
    m = max(m, __shfl_xor(m, 16));
    m = max(m, __shfl_xor(m, 32));
    any = (__shfl_xor((int)any, 16) | (int)any) != 0;
    any = (__shfl_xor((int)any, 32) | (int)any) != 0;

    // e_a of the legal squares (0 elsewhere) and their sum
    uint64_t S = 0;
    for (int T = 0; T < geo.OT; ++T) {
        const int o0 = 16 * T + 4 * g;
        const uint64_t lw = (T >> 2) < W ? words(2, T >> 2) : 0ull;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = o0 + r;
            const bool in_m = o < nn && ((lw >> (o & 63)) & 1u);
            const uint32_t e = in_m ? net_exp(m, zs[(4 * T + r) * 64 + lane], geo.policy_shift) : 0u;
            zs[(4 * T + r) * 64 + lane] = (int32_t)e;
            S += e;
        }
    }
    S += (uint64_t)__shfl_xor((unsigned long long)S, 16);
    S += (uint64_t)__shfl_xor((unsigned long long)S, 32);
    // the priors (a row without a legal square has S = 0 and is not divided)
    if (any) {
        for (int T = 0; T < geo.OT; ++T) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = (4 * T + r) * 64 + lane;
                zs[i] = net_prior((uint32_t)zs[i], S);
            }
        }
    }
    out.any = any;
    return out;
}

}  // namespace oth_dev
