// cnet.hip -- k_cnet_eval (oth_cnet_eval: the int8 residual convolutional network of cnet.hpp on rows in the
// exchange format) in one translation unit for every board size: N and W are run-time values, the channel
// count is a template parameter.
//
// A workgroup of four waves carries RB rows through the stem, the blocks and the head with the activations in
// the LDS (cnet_dev.hpp describes the mapping); a barrier separates two convs.  The integer softmax of a row is
// one wave's: the maximum and the sum cross the lanes by shuffles.
#include "cnet_dev.hpp"
#include "launch.hpp"

using namespace oth;

static_assert(sizeof(CnetParams) == sizeof(oth_cnet_params) && CNET_MAX_BLOCKS == OTH_CNET_MAX_BLOCKS &&
                  offsetof(CnetParams, shift) == offsetof(oth_cnet_params, shift) &&
                  offsetof(CnetParams, value_shift) == offsetof(oth_cnet_params, value_shift),
              "the header's struct and limits");

namespace oth_dev {

template <int C>
__global__ __launch_bounds__(CNET_THREADS) void k_cnet_eval(CnetGeo geo, int R, int RB,
                                                            const uint8_t* __restrict__ blob,
                                                            const uint64_t* __restrict__ boards,
                                                            const uint16_t* __restrict__ meta,
                                                            const uint64_t* __restrict__ legal,
                                                            int32_t* __restrict__ priors, int32_t* __restrict__ values,
                                                            int32_t* __restrict__ logits) {
    extern __shared__ uint4 lds[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        const uint64_t* hd = reinterpret_cast<const uint64_t*>(blob);
        uint64_t s0 = 0, s1 = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            s0 |= (uint64_t)geo.shifts[i] << (8 * i);
            s1 |= (uint64_t)geo.shifts[8 + i] << (8 * i);
        }
        if (hd[0] != geo.tag0() || hd[1] != geo.tag1() || hd[2] != s0 || hd[3] != s1) return;
    }
    const int nn = geo.nn, W = geo.W, P2 = geo.P2;
    const size_t image = (size_t)RB * P2 * C;
    uint8_t* h = reinterpret_cast<uint8_t*>(lds);
    uint8_t* t = h + image;
    uint8_t* pl = t + image;
    int32_t* zs = reinterpret_cast<int32_t*>(pl + (((size_t)RB * 3u * P2 + 15u) & ~(size_t)15u));
    int32_t* vsum = zs + (((size_t)RB * nn + 3u) & ~(size_t)3u);
    const int words = (int)(cnet_lds_bytes(geo, RB) / 16u);
    for (int i = tid; i < words; i += CNET_THREADS) lds[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    // the three planes of every row as bytes of 0 or 1 inside the halo
    const size_t row0 = (size_t)blockIdx.x * (size_t)RB;
    for (int i = tid; i < RB * 3 * nn; i += CNET_THREADS) {
        const int rb = i / (3 * nn), rest = i - rb * 3 * nn;
        const int p = rest / nn, a = rest - p * nn;
        const size_t row = row0 + (size_t)rb;
        if (row < (size_t)R) {
            const bool white = meta[row] & 1u;
            const uint64_t* src = p == 2 ? legal + row * W : boards + row * 2 * W + ((p == 0) == white ? W : 0);
            const int y = a / geo.n;
            pl[(rb * 3 + p) * P2 + (y + 1) * geo.NP + (a - y * geo.n) + 1] = (uint8_t)((src[a >> 6] >> (a & 63)) & 1u);
        }
    }
    __syncthreads();
    const int QT = RB * geo.ST;
    cnet_conv<C, CNET_STEM>(geo, blob + geo.off_stem(), geo.shift_stem, nullptr, h, pl, QT, wave, lane);
    __syncthreads();
    for (int k = 0; k < geo.B; ++k) {
        cnet_conv<C, CNET_FIRST>(geo, blob + geo.off_conv(2 * k), geo.shifts[2 * k], h, t, pl, QT, wave, lane);
        __syncthreads();
        cnet_conv<C, CNET_SECOND>(geo, blob + geo.off_conv(2 * k + 1), geo.shifts[2 * k + 1], t, h, pl, QT, wave, lane);
        __syncthreads();
    }
    cnet_head<C>(geo, blob, h, zs, vsum, QT, wave, lane);
    __syncthreads();
    // a row a wave: the value, the logits, the integer softmax over the legal squares
    for (int rb = wave; rb < RB; rb += CNET_WAVES) {
        const size_t row = row0 + (size_t)rb;
        if (row >= (size_t)R) break;
        const int32_t zv = *reinterpret_cast<const int32_t*>(blob + geo.off_bv()) + vsum[rb];
        if (lane == 0) {
            values[row] = net_value(zv, geo.value_shift);
            if (logits) logits[row * (size_t)(nn + 1) + nn] = zv;
        }
        int32_t z[4], m = INT32_MIN;
        bool in_m[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int a = lane + 64 * i;
            z[i] = a < nn ? zs[rb * nn + a] : 0;
            in_m[i] = a < nn && ((legal[row * W + (a >> 6)] >> (a & 63)) & 1u);
            if (a < nn && logits) logits[row * (size_t)(nn + 1) + a] = z[i];
            if (in_m[i]) m = max(m, z[i]);
        }
        const bool any = cnet_wave_max((int32_t)(in_m[0] | in_m[1] | in_m[2] | in_m[3])) != 0;
        m = cnet_wave_max(m);
        uint32_t e[4];
        uint64_t S = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            e[i] = in_m[i] ? net_exp(m, z[i], geo.policy_shift) : 0u;
            S += e[i];
        }
        S = cnet_wave_sum(S);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int a = lane + 64 * i;
            if (a < nn) priors[row * (size_t)nn + a] = any && in_m[i] ? net_prior(e[i], S) : 0;
        }
    }
}

}  // namespace oth_dev

namespace oth_host {

using namespace oth_dev;

namespace {
// a workgroup's LDS may pass the 64 KiB a kernel gets without asking (N = 16, C = 128: 83 KiB).  The attribute
// belongs to the current device's copy of the kernel, so it is asked for at every launch that needs it (N >= 14
// at C = 128), not once a process.
template <int C>
int cnet_allow_lds(size_t lds) {
    if (lds <= 64u * 1024u) return OTH_OK;
    const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_cnet_eval<C>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return err == hipSuccess ? OTH_OK : hip_fail(err, "oth_cnet_eval: hipFuncSetAttribute");
}
}  // namespace

// (of checked arguments, R >= 1)
int launch_cnet_eval(int n, const oth_cnet_params* p, int R, const void* blob, const uint64_t* boards,
                     const uint16_t* meta, const uint64_t* legal, int32_t* priors, int32_t* values, int32_t* logits,
                     hipStream_t st) {
    CnetParams cp;
    cp.channels = p->channels;
    cp.blocks = p->blocks;
    cp.shift_stem = p->shift_stem;
    for (int l = 0; l < 16; ++l) cp.shift[l] = p->shift[l];
    cp.shift_head = p->shift_head;
    cp.policy_shift = p->policy_shift;
    cp.value_shift = p->value_shift;
    const CnetGeo geo = cnet_geo(n, cp);
    const int RB = cnet_rows_per_block(geo.ST);
    const dim3 grid((unsigned)((R + RB - 1) / RB)), block(CNET_THREADS);
    const size_t lds = cnet_lds_bytes(geo, RB);
    const uint8_t* bl = reinterpret_cast<const uint8_t*>(blob);
    if (geo.C == 64) {
        if (int rc = cnet_allow_lds<64>(lds)) return rc;
        launch_k(k_cnet_eval<64>, grid, block, lds, st, geo, R, RB, bl, boards, meta, legal, priors, values, logits);
    } else {
        if (int rc = cnet_allow_lds<128>(lds)) return rc;
        launch_k(k_cnet_eval<128>, grid, block, lds, st, geo, R, RB, bl, boards, meta, legal, priors, values, logits);
    }
    return after_launch("oth_cnet_eval");
}

}  // namespace oth_host
