// net.hip -- k_net_eval (oth_net_eval: the int8 policy-value MLP of net.hpp on rows in the exchange format) in
// one translation unit for every board size: N and W are run-time values, the width is a template parameter.
//
// k_net_eval is a thin caller of net_dev.hpp's net_eval_tile (the mapping of a tile onto the matrix cores is
// described there): the rows come from global memory, the logits and the value go out from the head's pass, the
// priors from the LDS, each lane storing what it wrote there.
#include "net_dev.hpp"
#include "launch.hpp"

using namespace oth;

static_assert(sizeof(NetParams) == sizeof(oth_net_params) && NET_MAX_LAYERS == OTH_NET_MAX_LAYERS &&
                  NET_MAX_WIDTH == OTH_NET_MAX_WIDTH && NET_MAX_SHIFT == OTH_NET_MAX_SHIFT &&
                  NET_BIAS_MAX == OTH_NET_BIAS_MAX && NET_MAX_ROWS == OTH_NET_MAX_ROWS,
              "the header's struct and limits");

namespace oth_dev {

template <int KS>
__global__ __launch_bounds__(64) void k_net_eval(NetGeo geo, int R, const uint8_t* __restrict__ blob,
                                                 const uint64_t* __restrict__ boards,
                                                 const uint16_t* __restrict__ meta,
                                                 const uint64_t* __restrict__ legal, int32_t* __restrict__ priors,
                                                 int32_t* __restrict__ values, int32_t* __restrict__ logits) {
    extern __shared__ int32_t zs[];  // [OT][4][64]: logit r of head tile T of this lane, then its e_a, then its prior
    const int lane = (int)threadIdx.x, c = lane & 15, g = lane >> 4;
    const size_t row = (size_t)blockIdx.x * NET_ROWS + (size_t)c;
    const bool live = row < (size_t)R;
    const uint64_t* tags = reinterpret_cast<const uint64_t*>(blob);
    if (tags[0] != geo.tag0() || tags[1] != geo.tag1()) return;
    const int W = geo.W, nn = geo.nn;
    const bool white = live && (meta[row] & 1u);
    const NetTileOut out = net_eval_tile<KS>(
        geo, blob, zs, lane,
        [&](int p, int v) -> uint64_t {
            const uint64_t* src = p == 2 ? legal + row * W : boards + row * 2 * W + ((p == 0) == white ? W : 0);
            return live ? src[v] : 0ull;
        },
        [&](int o, int32_t z) {
            if (live && logits && o <= nn) logits[row * (size_t)(nn + 1) + o] = z;
            if (live && o == nn) values[row] = net_value(z, geo.value_shift);
        });
    if (OTH_NET_STOP == 1 || OTH_NET_STOP == 2) {
        if (live) values[row] = out.stop;
        return;
    }
    if (OTH_NET_STOP == 3) {
        if (live && g == 0) priors[row * (size_t)nn] = out.stop;
        return;
    }
    if (!live) return;
    for (int T = 0; T < geo.OT; ++T) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = 16 * T + 4 * g + r;
            if (o < nn) priors[row * (size_t)nn + o] = zs[(4 * T + r) * 64 + lane];
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
