// observe.hpp -- observations: k_observe (one thread per element), k_observe_w
// (one wave per group of boards, vector stores), and obs_stream / obs_tail, which
// the step kernels use to write the observation from their registers.
#pragma once
#include "state.hpp"

namespace oth_dev {

// A bfloat16 observation element (OTH_BF16).  The observations hold -1, 0 and
// +1 only, each exact in bfloat16: 0xBF80, 0x0000, 0x3F80.
struct obs_bf16 {
    uint16_t bits;
    obs_bf16() = default;
    __host__ __device__ explicit obs_bf16(int v) : bits(v == 0 ? 0u : (v > 0 ? 0x3F80u : 0xBF80u)) {}
};
static_assert(sizeof(obs_bf16) == 2, "a bfloat16");

template <typename T>
__device__ __forceinline__ void put(void* out, size_t i, int v) {
    reinterpret_cast<T*>(out)[i] = (T)v;
}

// planes of an observation layout (OTH_OBS_*)
__host__ __device__ constexpr int obs_planes(int layout) {
    return layout == OTH_OBS_BOARD_LEGAL ? 2 : (layout == OTH_OBS_MAKE_STATE ? 4 : 1);
}

// One thread per output element, (E, planes, N, N) row-major: coalesced stores.
template <int N>
__global__ __launch_bounds__(BLOCK) void k_observe(const uint64_t* __restrict__ boards,
                                                   const uint16_t* __restrict__ meta,
                                                   const uint64_t* __restrict__ legal, int E, int layout, int dtype,
                                                   void* __restrict__ out) {
    constexpr int W = Geo<N>::W;
    constexpr int NN = N * N;
    // (obs_planes(layout) written out: through the call the plane tests below become 64-bit compares)
    const int planes = layout == OTH_OBS_BOARD_LEGAL ? 2 : (layout == OTH_OBS_MAKE_STATE ? 4 : 1);
    const size_t total = (size_t)E * planes * NN;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLOCK) {
        const int a = (int)(i % NN);
        const size_t rest = i / NN;
        const int plane = (int)(rest % planes);
        const size_t e = rest / planes;
        const int wi = a / 64, bi = a % 64;
        const int isb = (int)((boards[e * 2 * W + wi] >> bi) & 1u);
        const int isw = (int)((boards[e * 2 * W + W + wi] >> bi) & 1u);
        const uint32_t m = meta[e];
        const bool tw = (m & M_TURN_WHITE) != 0;
        int v;
        if (layout == OTH_OBS_ABSOLUTE) {
            v = isw - isb;
        } else if (layout == OTH_OBS_LEGAL) {
            v = (int)((legal[e * W + wi] >> bi) & 1u);
        } else if (layout == OTH_OBS_MAKE_STATE) {
            if (plane == 0) {
                v = isb;
            } else if (plane == 1) {
                v = isw;
            } else if (plane == 2) {
                v = tw ? 1 : 0;
            } else {  // util.py:55: the legal plane only when >= 2 moves
                int cnt = 0;
#pragma unroll
                for (int k = 0; k < W; ++k) cnt += popc64(legal[e * W + k]);
                v = cnt > 1 ? (int)((legal[e * W + wi] >> bi) & 1u) : 0;
            }
        } else {
            if (plane == 0) {
                v = tw ? (isw - isb) : (isb - isw);  // othello.py:364-369
            } else {
                v = (int)((legal[e * W + wi] >> bi) & 1u);
            }
        }
        switch (dtype) {
            case OTH_I8: put<int8_t>(out, i, v); break;
            case OTH_I32: put<int32_t>(out, i, v); break;
            case OTH_I64: put<int64_t>(out, i, v); break;
            case OTH_F32: put<float>(out, i, v); break;
            case OTH_BF16: put<obs_bf16>(out, i, v); break;
            default: put<double>(out, i, v); break;
        }
    }
}

// A quad of 4 consecutive squares of one plane as one vector store (16 B for
// f32 / i32, 8 B for bf16, 4 B for i8, 2 x 16 B for the 8-byte types): k_observe_w's unit
// (the 8-byte types take pairs of squares instead, OTH_OBS_PAIR8).
// (as streaming stores: 65,536 boards 2-3 % slower, 1,048,576 int64 boards 104 -> 250 us;
// profiles/r04/d/ab_obs_nt.jsonl)
template <typename T>
__device__ __forceinline__ void put_quad(T* out, uint32_t q, int v0, int v1, int v2, int v3) {
    if constexpr (sizeof(T) == 1) {
        const uint32_t x = (uint32_t)(uint8_t)(int8_t)v0 | ((uint32_t)(uint8_t)(int8_t)v1 << 8) |
                           ((uint32_t)(uint8_t)(int8_t)v2 << 16) | ((uint32_t)(uint8_t)(int8_t)v3 << 24);
        reinterpret_cast<uint32_t*>(out)[q] = x;
    } else if constexpr (sizeof(T) == 2) {
        uint2 x;
        x.x = (uint32_t)T(v0).bits | ((uint32_t)T(v1).bits << 16);
        x.y = (uint32_t)T(v2).bits | ((uint32_t)T(v3).bits << 16);
        reinterpret_cast<uint2*>(out)[q] = x;
    } else if constexpr (sizeof(T) == 4) {
        using V4 = typename std::conditional<std::is_same<T, float>::value, float4, int4>::type;
        V4 x;
        x.x = (T)v0;
        x.y = (T)v1;
        x.z = (T)v2;
        x.w = (T)v3;
        reinterpret_cast<V4*>(out)[q] = x;
    } else {
        using V2 = typename std::conditional<std::is_same<T, double>::value, double2, longlong2>::type;
        V2 a, b;
        a.x = (T)v0;
        a.y = (T)v1;
        b.x = (T)v2;
        b.y = (T)v3;
        reinterpret_cast<V2*>(out)[2 * (size_t)q] = a;
        reinterpret_cast<V2*>(out)[2 * (size_t)q + 1] = b;
    }
}

// S one- or two-byte observation elements of one unit (+1 where pos, -1 where
// neg, 0 elsewhere: bit j of the masks is square j of the unit) as ONE store of
// S * sizeof(T) bytes.  Each dword spreads 4 bits into bytes (bit i of x < 16
// lands in byte i of x * 0x204081 & 0x01010101) or 2 bits into halves (x * 0x8001
// & 0x10001), then scales: 0xFF (int8 -1), 0x3F80 / 0xBF80 (bf16 +1 / -1).
template <typename T, int S>
__device__ __forceinline__ void put_narrow(T* out, uint32_t g, uint32_t pos, uint32_t neg) {
    static_assert(sizeof(T) <= 2 && (S * sizeof(T)) % 4 == 0 && S * sizeof(T) <= 16, "one store of 4 to 16 bytes");
    constexpr int D = (int)(S * sizeof(T) / 4);
    uint32_t d[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        if constexpr (sizeof(T) == 1) {
            const uint32_t p = (pos >> (4 * k)) & 0xFu, n = (neg >> (4 * k)) & 0xFu;
            d[k] = ((p * 0x204081u) & 0x01010101u) | (((n * 0x204081u) & 0x01010101u) * 0xFFu);
        } else {
            const uint32_t p = (pos >> (2 * k)) & 3u, n = (neg >> (2 * k)) & 3u;
            d[k] = ((p * 0x8001u) & 0x10001u) * 0x3F80u | ((n * 0x8001u) & 0x10001u) * 0xBF80u;
        }
    }
    if constexpr (D == 4) {
        reinterpret_cast<uint4*>(out)[g] = make_uint4(d[0], d[1], d[2], d[3]);
    } else if constexpr (D == 2) {
        reinterpret_cast<uint2*>(out)[g] = make_uint2(d[0], d[1]);
    } else {
        reinterpret_cast<uint32_t*>(out)[g] = d[0];
    }
}

#ifndef OTH_OBS_PAIR8
// 8-byte observations by pairs of squares, one 16-B store per lane (1 KiB
// contiguous per store instruction) instead of quads in two 16-B stores (each
// instruction half of a 2-KiB span): oth_step_observe with its int64 board at
// 65,536 8x8 boards 11.05 -> 8.80 us per graphed ply (torch's fill_ of the same
// tensor: 8.95; profiles/r05/i/ab_step_obs.json)
#define OTH_OBS_PAIR8 1
#endif
// obs_stream's squares per lane and store for NN squares of esize-byte elements
// (below), and the byte alignment the output needs for them
__host__ __device__ constexpr int obs_unit(int NN, int esize) {
    return esize == 8 ? (OTH_OBS_PAIR8 ? 2 : 4) : (NN % (16 / esize) == 0 ? 16 / esize : 4);
}
__host__ __device__ constexpr int obs_align(int NN, int esize) {
    return obs_unit(NN, esize) * esize > 4 * esize ? obs_unit(NN, esize) * esize : 4 * esize;
}
template <int LAYOUT>
constexpr bool obs_needs_legal() {
    return LAYOUT == OTH_OBS_BOARD_LEGAL || LAYOUT == OTH_OBS_MAKE_STATE || LAYOUT == OTH_OBS_LEGAL;
}
// the board facts the observation needs beside its words: bit 0 white to move,
// bit 1 more than one legal move (util.py:55's make_state condition)
template <int W>
__device__ __forceinline__ uint32_t obs_flags(uint32_t m, const uint64_t (&lw)[W]) {
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) cnt += popc64(lw[k]);
    return ((m & M_TURN_WHITE) ? 1u : 0u) | (cnt > 1 ? 2u : 0u);
}

// The observation (E, planes, N, N) of nb <= BPW consecutive boards whose words
// the wave holds -- board kb's black / white / possible_moves words and its
// obs_flags in lane kb * LS (LS lanes per board) -- streamed into their
// contiguous output region `base` (nb x planes x N*N/4 quads), one 64-quad
// vector store per step, each lane taking the words of the board its quad
// belongs to from that board's lane (ds_bpermute).  Every lane of the wave
// must take part (ds_bpermute reads an inactive source lane as 0).  Used by
// k_observe_w (the boards loaded from HBM) and by the step kernels' fused
// observation (oth_step_observe / oth_sample_step_observe: the boards as the
// step left them in registers).
template <int N, int LAYOUT, typename T, int BPW, int LS = 1>
__device__ __forceinline__ void obs_stream(const uint64_t (&bw)[Geo<N>::W], const uint64_t (&ww)[Geo<N>::W],
                                           const uint64_t (&lw)[Geo<N>::W], uint32_t fl, int nb,
                                           T* __restrict__ base) {
    static_assert(BPW * LS <= 64, "the wave holds its boards");
    constexpr int W = Geo<N>::W;
    constexpr int NN = N * N;
    static_assert(NN % 4 == 0, "quads of squares");
    constexpr int Q = NN / 4;
    constexpr int PQ = obs_planes(LAYOUT) * Q;  // quads per board
    constexpr bool NEED_L = obs_needs_legal<LAYOUT>();
    const int lane = threadIdx.x & 63;
    const int total = nb * PQ;
    auto fetch = [&](const uint64_t (&x)[W], int kb, int wi) __attribute__((always_inline)) {
        uint64_t r = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const uint64_t y = (uint64_t)__shfl((unsigned long long)x[k], kb * LS);
            r = wi == k ? y : r;
        }
        return r;
    };
    // every lane takes part in every step (ds_bpermute reads an inactive source lane
    // as 0): the last step's lanes past the region clamp their quad and skip the store.
    // Measured and not kept (1,048,576 boards, make_state f32; a plain torch fill of the
    // same tensor: 155 us, ours 219): the waves starting their regions at different
    // steps 217.8 -> 225.8 us; boards dealt to the waves with the grid's stride (the
    // resident waves store into one window) 219.6 -> 264.3; the step's board words by
    // v_readlane 218.9 -> 217.5 (and +-0 again on the branch-free body below); the loop
    // unrolled by 4 +-0 (by 2 / 4 on the branch-free body: +-0, profiles/r04/obs/ab_unroll_bf.jsonl); 128 / 256 boards per wave (every wave resident at once, all
    // loads first) 218.8 -> 216.6 / 234.4, and at 262,144 boards 46.5 -> 57.6 / 110.3
    // (profiles/r04/obs/)
    // S squares per lane and store: 16 bytes a lane where a plane divides into such
    // units -- 16 squares of int8, 8 of bf16, quads of the 4-byte types, and for the
    // 8-byte types under OTH_OBS_PAIR8 pairs (one 16-B store per lane, so each store
    // instruction writes 1 KiB contiguous instead of two half-filled 2-KiB spans) --
    // else quads.  One- and two-byte units are packed from their bit masks
    // (put_narrow): at 65,536 8x8 boards the learners' fused ply with its make_state
    // 15.43 -> 10.03 us per graphed ply in int8 (quads: a 4-B store per lane; the
    // sample-step alone 6.2), 17.25 -> 13.34 in bf16; k_observe_w make_state int8
    // 9.54 -> 5.36 us, 1,048,576 boards 86.6 -> 50.0 (profiles/r06/e)
    constexpr int S = obs_unit(NN, (int)sizeof(T));
    constexpr bool NARROW = sizeof(T) <= 2;
    constexpr uint32_t UQ = (uint32_t)(NN / S), UB = (uint32_t)obs_planes(LAYOUT) * UQ;  // units per plane / board
    constexpr uint32_t SM = (1u << S) - 1u;
    const int totalu = nb * (int)UB;
    (void)total;
    for (int g0 = 0; g0 < totalu; g0 += 64) {
        const uint32_t g = (uint32_t)(g0 + lane < totalu ? g0 + lane : totalu - 1);
        const uint32_t kb = g / UB, rr = g - kb * UB;
        const uint32_t plane = rr / UQ, q = rr - plane * UQ;
        const uint32_t a0 = S * q, wi = a0 / 64, bi = a0 % 64;  // S | 64: a unit never straddles words
        // (a probe storing values made from g alone, nothing fetched: k_observe_w at 65,536 /
        // 1,048,576 boards, make_state f32 13.1 -> 12.5 / 208.7 -> 187.3 us, int64 board
        // 7.9 -> 7.8 / 100.5 -> 89.8; profiles/r05/l/ab_obs_cst.jsonl)
        const uint64_t xb = fetch(bw, (int)kb, (int)wi), xw = fetch(ww, (int)kb, (int)wi);
        const uint32_t flk = (uint32_t)__shfl((int)fl, (int)kb * LS);
        const bool tw = (flk & 1u) != 0;
        uint64_t xl = 0;
        if constexpr (NEED_L) xl = fetch(lw, (int)kb, (int)wi);
        // the lanes of one store cover several planes: each lane's plane word is
        // picked by masks, not branches (the compiler had made the plane choice
        // branches, so the wave ran every plane's path in turn with exec-mask SALU
        // between them): make_state f32 at 65,536 / 262,144 / 1,048,576 boards
        // 13.75 -> 12.79 / 46.6 -> 41.5 / 219.8 -> 208.3 us, int64 board 1,048,576
        // 104.7 -> 102.4 (profiles/r04/obs/ab_branchfree.jsonl)
        if constexpr (NARROW) {  // +1 where pos, -1 where neg, packed a dword at a time
            uint32_t pos, neg = 0u;
            if constexpr (LAYOUT == OTH_OBS_LEGAL) {
                pos = (uint32_t)(xl >> bi) & SM;
            } else if constexpr (LAYOUT == OTH_OBS_ABSOLUTE) {
                pos = (uint32_t)(xw >> bi) & SM;
                neg = (uint32_t)(xb >> bi) & SM;
            } else if constexpr (LAYOUT == OTH_OBS_MAKE_STATE) {
                const uint64_t m0 = 0ull - (uint64_t)(plane == 0u), m1 = 0ull - (uint64_t)(plane == 1u);
                const uint64_t m2 = 0ull - (uint64_t)(plane == 2u && tw), m3 = 0ull - (uint64_t)(plane == 3u && (flk & 2u));
                pos = (uint32_t)(((xb & m0) | (xw & m1) | (xl & m3) | m2) >> bi) & SM;
            } else {
                const uint64_t xm = tw ? xw : xb, xo = tw ? xb : xw;
                const bool p1 = plane != 0u;
                pos = (uint32_t)((p1 ? xl : xm) >> bi) & SM;
                neg = p1 ? 0u : (uint32_t)(xo >> bi) & SM;
            }
            if (g0 + lane < totalu) put_narrow<T, S>(base, g, pos, neg);
            continue;
        }
        int v[4] = {0, 0, 0, 0};
        if constexpr (LAYOUT == OTH_OBS_LEGAL) {  // possible_moves
            const uint32_t nl = (uint32_t)(xl >> bi) & SM;
#pragma unroll
            for (int j = 0; j < S; ++j) v[j] = (int)((nl >> j) & 1u);
        } else if constexpr (LAYOUT == OTH_OBS_ABSOLUTE) {  // othello.py:257
            const uint32_t nbk = (uint32_t)(xb >> bi) & SM, nwk = (uint32_t)(xw >> bi) & SM;
#pragma unroll
            for (int j = 0; j < S; ++j) v[j] = (int)((nwk >> j) & 1u) - (int)((nbk >> j) & 1u);
        } else if constexpr (LAYOUT == OTH_OBS_MAKE_STATE) {  // util.py:48-74
            const uint64_t m0 = 0ull - (uint64_t)(plane == 0u), m1 = 0ull - (uint64_t)(plane == 1u);
            const uint64_t m2 = 0ull - (uint64_t)(plane == 2u && tw), m3 = 0ull - (uint64_t)(plane == 3u && (flk & 2u));
            const uint32_t bits = (uint32_t)(((xb & m0) | (xw & m1) | (xl & m3) | m2) >> bi) & SM;
#pragma unroll
            for (int j = 0; j < S; ++j) v[j] = (int)((bits >> j) & 1u);
        } else {  // othello.py:363-376: mover +1, opponent -1; plane 1 the legal squares
            const uint64_t xm = tw ? xw : xb, xo = tw ? xb : xw;
            const uint32_t mv = (uint32_t)(xm >> bi) & SM, op = (uint32_t)(xo >> bi) & SM;
            const uint32_t nl = (uint32_t)(xl >> bi) & SM;
            const bool p1 = plane != 0u;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const int b = (int)((mv >> j) & 1u) - (int)((op >> j) & 1u);
                v[j] = p1 ? (int)((nl >> j) & 1u) : b;
            }
        }
        if (g0 + lane < totalu) {
            if constexpr (S == 2) {
                using V2 = typename std::conditional<std::is_same<T, double>::value, double2, longlong2>::type;
                V2 x;
                x.x = (T)v[0];
                x.y = (T)v[1];
                reinterpret_cast<V2*>(base)[g] = x;
            } else {
                put_quad<T>(base, g, v[0], v[1], v[2], v[3]);
            }
        }
    }
}

// k_observe_w: the same values as k_observe, one wave per BPW consecutive
// boards.  Each lane loads one board (coalesced), then the wave streams the
// boards' output region (obs_stream).  One board per wave (round 2's
// k_observe_q, each wave waiting on its own board's loads before one 1-KiB
// store) reached 2.6 TB/s for make_state f32 at 1,048,576 boards; one wave's
// loads feeding 64 boards' stores, 5.0 (a plain fill: 6.9).  BPW boards per wave:
// 16 below 262,144 boards (four times the waves of 64, each streaming a quarter
// of the region, so the store streams start sooner and more of them are in
// flight); from there 64, and once the output exceeds 384 MiB as many as fill
// about 4 KiB of output (launch_observe_w: make_state f32 at 1,048,576 boards
// 5.3 -> 6.0 TB/s with 4 boards a wave).
template <int N, int LAYOUT, typename T, int BPW = 64>
__global__ __launch_bounds__(BLOCK) void k_observe_w(const uint64_t* __restrict__ boards,
                                                     const uint16_t* __restrict__ meta,
                                                     const uint64_t* __restrict__ legal, int E, T* __restrict__ out) {
    static_assert(BPW == 4 || BPW == 8 || BPW == 16 || BPW == 32 || BPW == 64, "boards per wave");
    constexpr int W = Geo<N>::W;
    constexpr int PQ = obs_planes(LAYOUT) * N * N / 4;  // quads per board
    const int lane = threadIdx.x & 63;
    const long long e0 = ((long long)blockIdx.x * BLOCK + threadIdx.x - lane) / 64 * BPW;  // the wave's first board
    if (e0 >= E) return;                                                                 // wave-uniform
    const long long e = lane < BPW ? e0 + lane : E;  // lanes past BPW load nothing
    uint64_t bw[W], ww[W], lw[W];
    uint32_t fl = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) bw[k] = ww[k] = lw[k] = 0;
    if (e < E) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            bw[k] = boards[(size_t)e * 2 * W + k];
            ww[k] = boards[(size_t)e * 2 * W + W + k];
            if constexpr (obs_needs_legal<LAYOUT>()) lw[k] = legal[(size_t)e * W + k];
        }
        fl = obs_flags<W>(meta[e], lw);
    }
    const int nb = (int)(E - e0 < BPW ? E - e0 : BPW);
    obs_stream<N, LAYOUT, T, BPW, 1>(bw, ww, lw, fl, nb, out + (size_t)e0 * PQ * 4);
}

// The fused observation of the step kernels (oth_step_observe,
// oth_sample_step_observe): obs_stream for a runtime layout and dtype (kernel
// arguments, so the switch is a scalar branch taken once per wave), into the
// region of the wave's first board e0.  layout < 0: no observation.  Only
// N*N % 4 == 0 (the quad stores); the C ABI takes two launches for other N.
template <int N, int BPW, int LS>
__device__ __forceinline__ void obs_tail(int layout, int dtype, void* __restrict__ out, long long e0,
                                         const uint64_t (&bw)[Geo<N>::W], const uint64_t (&ww)[Geo<N>::W],
                                         const uint64_t (&lw)[Geo<N>::W], uint32_t m, int nb) {
    if constexpr ((N * N) % 4 == 0) {
        if (layout < 0 || nb <= 0) return;
        const uint32_t fl = obs_flags<Geo<N>::W>(m, lw);
        // (the layout switch written out, not through the launchers' with_layout: through a
        // helper the stores of every kernel with this tail come out in other registers)
        auto by_type = [&](auto LC) __attribute__((always_inline)) {
            constexpr int LAY = decltype(LC)::value;
            constexpr size_t PER = (size_t)obs_planes(LAY) * N * N;  // elements per board
            switch (dtype) {
                case OTH_I8:
                    obs_stream<N, LAY, int8_t, BPW, LS>(bw, ww, lw, fl, nb, (int8_t*)out + e0 * PER);
                    break;
                case OTH_I32:
                    obs_stream<N, LAY, int32_t, BPW, LS>(bw, ww, lw, fl, nb, (int32_t*)out + e0 * PER);
                    break;
                case OTH_I64:
                    obs_stream<N, LAY, long long, BPW, LS>(bw, ww, lw, fl, nb, (long long*)out + e0 * PER);
                    break;
                case OTH_F32:
                    obs_stream<N, LAY, float, BPW, LS>(bw, ww, lw, fl, nb, (float*)out + e0 * PER);
                    break;
                case OTH_BF16:
                    obs_stream<N, LAY, obs_bf16, BPW, LS>(bw, ww, lw, fl, nb, (obs_bf16*)out + e0 * PER);
                    break;
                default:
                    obs_stream<N, LAY, double, BPW, LS>(bw, ww, lw, fl, nb, (double*)out + e0 * PER);
                    break;
            }
        };
        switch (layout) {
            case OTH_OBS_BOARD: by_type(std::integral_constant<int, OTH_OBS_BOARD>{}); break;
            case OTH_OBS_BOARD_LEGAL: by_type(std::integral_constant<int, OTH_OBS_BOARD_LEGAL>{}); break;
            case OTH_OBS_MAKE_STATE: by_type(std::integral_constant<int, OTH_OBS_MAKE_STATE>{}); break;
            case OTH_OBS_ABSOLUTE: by_type(std::integral_constant<int, OTH_OBS_ABSOLUTE>{}); break;
            default: by_type(std::integral_constant<int, OTH_OBS_LEGAL>{}); break;
        }
    }
}

}  // namespace oth_dev
