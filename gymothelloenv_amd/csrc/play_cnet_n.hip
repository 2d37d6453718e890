// play_cnet_n.hip -- k_play_cnet (oth_play_cnet, oth_reset_vs_cnet, oth_step_vs_cnet: the convolutional network as
// a player, play_cnet.hpp) in a translation unit of its own per board size (-DOTH_N=4 .. 16), like play_net_n.hip.
// The mode is a kernel argument, so a unit holds one kernel a channel count: two.
#include "play_cnet.hpp"
#include "launch.hpp"

#ifndef OTH_N
#error "compile with -DOTH_N=<board size>"
#endif

using namespace oth;
using namespace oth_dev;

static_assert(sizeof(oth_cnet_policy) == sizeof(oth_cnet_params) + 24 && offsetof(oth_cnet_policy, blob) == sizeof(oth_cnet_params),
              "the header's struct");

namespace oth_host {

namespace {
PlayCnetSide side_of(int n, const oth_cnet_policy* p) {
    CnetParams cp;
    cp.channels = p->params.channels;
    cp.blocks = p->params.blocks;
    cp.shift_stem = p->params.shift_stem;
    for (int l = 0; l < 16; ++l) cp.shift[l] = p->params.shift[l];
    cp.shift_head = p->params.shift_head;
    cp.policy_shift = p->params.policy_shift;
    cp.value_shift = p->params.value_shift;
    return PlayCnetSide{cnet_geo(n, cp), reinterpret_cast<const uint8_t*>(p->blob), p->sample_discs};
}
bool same_head(const CnetGeo& a, const CnetGeo& b) {
    uint8_t ha[CNET_HEAD_BYTES], hb[CNET_HEAD_BYTES];
    a.head(ha);
    b.head(hb);
    for (int i = 0; i < CNET_HEAD_BYTES; ++i)
        if (ha[i] != hb[i]) return false;
    return true;
}
// a workgroup's LDS may pass the 64 KiB a kernel gets without asking (N >= 14 at C = 128): the attribute belongs
// to the current device's copy of the kernel, so it is asked for at every launch that needs it, before the
// launch is issued (or recorded, under stream capture)
template <int N, int C>
int play_cnet_allow_lds(size_t lds) {
    if (lds <= 64u * 1024u) return OTH_OK;
    const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_play_cnet<N, C>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return err == hipSuccess ? OTH_OK : hip_fail(err, "oth_play_cnet: hipFuncSetAttribute");
}
}  // namespace

template <int N>
int launch_play_cnet(oth_env* env, int mode, const oth_cnet_policy* black, const oth_cnet_policy* white, int n_plies,
                     const int32_t* act_in, const int8_t* prot, const uint8_t* mask, int32_t* actions, int32_t* rewards,
                     uint8_t* dones, int32_t* plies, uint64_t ctr, hipStream_t st) {
    static_assert(OTH_PLAY_SEARCH_PLAY == PS_PLAY && OTH_PLAY_SEARCH_STEP_VS == PS_STEP_VS &&
                      OTH_PLAY_SEARCH_RESET_VS == PS_RESET_VS, "the launchers' modes are the kernels'");
    const PlayCnetSide sb = side_of(N, black), sw = side_of(N, white);
    const int RB = cnet_rows_per_block(sb.geo.ST);
    const long long groups = ((long long)env->E + RB - 1) / RB;
    const int same = sb.blob == sw.blob && same_head(sb.geo, sw.geo) ? 1 : 0;
    const Rng rng{env->seed, env->id_base, env->init_rand, env->cur_off, 0};
    const dim3 grid((unsigned)groups), block(CNET_THREADS);
    const size_t lds = play_cnet_lds_bytes(sb.geo, RB);
#define OTH_PLAY_CNET_CASE(C)                                                                                        \
    {                                                                                                                \
        if (int rc = play_cnet_allow_lds<N, C>(lds)) return rc;                                                      \
        launch_k(k_play_cnet<N, C>, grid, block, lds, st, env->boards, env->meta, env->legal, env->E, env->flags,    \
                 mode, PlayCnetSides{{sb, sw}}, same, n_plies, act_in, prot, mask, actions, rewards, dones, plies,   \
                 env->wdl, env->wdl_vs, rng, ctr);                                                                   \
    }
    if (sb.geo.C == 64) OTH_PLAY_CNET_CASE(64)
    else if (sb.geo.C == 128) OTH_PLAY_CNET_CASE(128)
    else return fail(OTH_EINVAL, "channels must be 64 or 128");
#undef OTH_PLAY_CNET_CASE
    return after_launch("oth_play_cnet");
}

template int launch_play_cnet<OTH_N>(oth_env*, int, const oth_cnet_policy*, const oth_cnet_policy*, int, const int32_t*,
                                     const int8_t*, const uint8_t*, int32_t*, int32_t*, uint8_t*, int32_t*, uint64_t,
                                     hipStream_t);

}  // namespace oth_host
