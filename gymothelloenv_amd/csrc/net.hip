// net.hip -- k_net_eval (oth_net_eval: the int8 policy-value MLP of net.hpp on rows in the exchange format) in
// one translation unit for every board size: N and W are run-time values, the width is a template parameter.
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
#include "net.hpp"
#include "launch.hpp"

using namespace oth;

static_assert(sizeof(NetParams) == sizeof(oth_net_params) && NET_MAX_LAYERS == OTH_NET_MAX_LAYERS &&
                  NET_MAX_WIDTH == OTH_NET_MAX_WIDTH && NET_MAX_SHIFT == OTH_NET_MAX_SHIFT &&
                  NET_BIAS_MAX == OTH_NET_BIAS_MAX && NET_MAX_ROWS == OTH_NET_MAX_ROWS,
              "the header's struct and limits");

namespace oth_dev {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int NET_ROWS = 16;  // rows a wave

// tools/probe_net.py's variants, never the shipped library: 1, 2, 3 end the kernel after layer 0, after the
// hidden layers, after the head's logits (one word of what was computed is stored, so that it is computed)
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

template <int KS>
__global__ __launch_bounds__(64) void k_net_eval(NetGeo geo, int R, const uint8_t* __restrict__ blob,
                                                 const uint64_t* __restrict__ boards,
                                                 const uint16_t* __restrict__ meta,
                                                 const uint64_t* __restrict__ legal, int32_t* __restrict__ priors,
                                                 int32_t* __restrict__ values, int32_t* __restrict__ logits) {
    extern __shared__ int32_t zs[];  // [OT][4][64]: logit r of head tile T of this lane, then its e_a
    const int lane = (int)threadIdx.x, c = lane & 15, g = lane >> 4;
    const size_t row = (size_t)blockIdx.x * NET_ROWS + (size_t)c;
    const bool live = row < (size_t)R;
    const uint64_t* tags = reinterpret_cast<const uint64_t*>(blob);
    if (tags[0] != geo.tag0() || tags[1] != geo.tag1()) return;
    const int W = geo.W, nn = geo.nn;
    const bool white = live && (meta[row] & 1u);

    // layer 0: every output tile's accumulator live, a k-step a word of a plane
    v4i acc[4 * KS];
    {
        const uint8_t* bias = blob + geo.off_bias(0);
        const uint8_t* tiles = blob + geo.off_tiles(0);
#pragma unroll
        for (int T = 0; T < 4 * KS; ++T) acc[T] = *reinterpret_cast<const v4i*>(bias + 64 * T + 16 * g);
        for (int s = 0; s < geo.K0S; ++s) {
            const int p = s / W, v = s - p * W;
            const uint64_t* src = p == 2 ? legal + row * W : boards + row * 2 * W + ((p == 0) == white ? W : 0);
            const uint64_t word = live ? src[v] : 0ull;
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
        int x = 0;
#pragma unroll
        for (int q = 0; q < KS; ++q) x ^= h[q][0] ^ h[q][1] ^ h[q][2] ^ h[q][3];
        if (live) values[row] = x;
        return;
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
        int x = 0;
#pragma unroll
        for (int q = 0; q < KS; ++q) x ^= h[q][0] ^ h[q][1] ^ h[q][2] ^ h[q][3];
        if (live) values[row] = x;
        return;
    }

    // the head: logit o = 16 T + 4 g + r of row c, kept in the LDS; the value; the largest legal logit
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
        const uint64_t lw = live && (T >> 2) < W ? legal[row * W + (T >> 2)] : 0ull;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = o0 + r;
            zs[(4 * T + r) * 64 + lane] = z[r];
            if (live && logits && o <= nn) logits[row * (size_t)(nn + 1) + o] = z[r];
            if (live && o == nn) values[row] = net_value(z[r], geo.value_shift);
            if (o < nn && ((lw >> (o & 63)) & 1u)) {
                any = true;
                m = z[r] > m ? z[r] : m;
            }
        }
    }
    if (OTH_NET_STOP == 3) {
        if (live && g == 0) priors[row * (size_t)nn] = m;
        return;
    }
    m = max(m, __shfl_xor(m, 16));
    m = max(m, __shfl_xor(m, 32));
    any = (__shfl_xor((int)any, 16) | (int)any) != 0;
    any = (__shfl_xor((int)any, 32) | (int)any) != 0;

    // e_a of the legal squares (0 elsewhere) and their sum
    uint64_t S = 0;
    for (int T = 0; T < geo.OT; ++T) {
        const int o0 = 16 * T + 4 * g;
        const uint64_t lw = live && (T >> 2) < W ? legal[row * W + (T >> 2)] : 0ull;
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
    if (!live) return;
    for (int T = 0; T < geo.OT; ++T) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = 16 * T + 4 * g + r;
            if (o < nn) priors[row * (size_t)nn + o] = any ? net_prior((uint32_t)zs[(4 * T + r) * 64 + lane], S) : 0;
        }
    }
}

}  // namespace oth_dev

namespace oth_host {

using namespace oth_dev;

// (of checked arguments, R >= 1)
int launch_net_eval(int n, const oth_net_params* p, int R, const void* blob, const uint64_t* boards,
                    const uint16_t* meta, const uint64_t* legal, int32_t* priors, int32_t* values, int32_t* logits,
                    hipStream_t st) {
    NetParams np;
    np.layers = p->layers;
    np.width = p->width;
    for (int l = 0; l < 4; ++l) np.shift[l] = p->shift[l];
    np.policy_shift = p->policy_shift;
    np.value_shift = p->value_shift;
    const NetGeo geo = net_geo(n, np);
    const dim3 grid((unsigned)((R + NET_ROWS - 1) / NET_ROWS)), block(64);
    const size_t lds = (size_t)geo.OT * 4 * 64 * sizeof(int32_t);
    const uint8_t* bl = reinterpret_cast<const uint8_t*>(blob);
    switch (geo.KS) {
#define OTH_NET_CASE(K)                                                                                              \
    case K:                                                                                                          \
        launch_k(k_net_eval<K>, grid, block, lds, st, geo, R, bl, boards, meta, legal, priors, values, logits);      \
        break;
        OTH_NET_CASE(1)
        OTH_NET_CASE(2)
        OTH_NET_CASE(3)
        OTH_NET_CASE(4)
        OTH_NET_CASE(5)
        OTH_NET_CASE(6)
        OTH_NET_CASE(7)
        OTH_NET_CASE(8)
#undef OTH_NET_CASE
        default: return fail(OTH_EINVAL, "width must be a multiple of 64 in [64, 512]");
    }
    return after_launch("oth_net_eval");
}

}  // namespace oth_host
