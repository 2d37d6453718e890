// play_net_n.hip -- k_play_net (oth_play_net, oth_reset_vs_net, oth_step_vs_net: the network as a player,
// play_net.hpp) in a translation unit of its own per board size (-DOTH_N=4 .. 16), like play_search_n.hip.  The
// mode is a kernel argument, so a unit holds one kernel a width: eight.
#include "play_net.hpp"
#include "launch.hpp"

#ifndef OTH_N
#error "compile with -DOTH_N=<board size>"
#endif

using namespace oth;
using namespace oth_dev;

static_assert(NET_SAMPLE_DISCS_MAX == OTH_NET_SAMPLE_DISCS_MAX && sizeof(oth_net_policy) == 56, "the header's struct and limit");

namespace oth_host {

namespace {
PlayNetSide side_of(int n, const oth_net_policy* p) {
    NetParams np;
    np.layers = p->params.layers;
    np.width = p->params.width;
    for (int l = 0; l < 4; ++l) np.shift[l] = p->params.shift[l];
    np.policy_shift = p->params.policy_shift;
    np.value_shift = p->params.value_shift;
    return PlayNetSide{net_geo(n, np), reinterpret_cast<const uint8_t*>(p->blob), p->sample_discs};
}
}  // namespace

template <int N>
int launch_play_net(oth_env* env, int mode, const oth_net_policy* black, const oth_net_policy* white, int n_plies,
                    const int32_t* act_in, const int8_t* prot, const uint8_t* mask, int32_t* actions, int32_t* rewards,
                    uint8_t* dones, int32_t* plies, uint64_t ctr, hipStream_t st) {
    static_assert(OTH_PLAY_SEARCH_PLAY == PS_PLAY && OTH_PLAY_SEARCH_STEP_VS == PS_STEP_VS &&
                      OTH_PLAY_SEARCH_RESET_VS == PS_RESET_VS, "the launchers' modes are the kernels'");
    const long long groups = ((long long)env->E + PLAY_NET_GROUP - 1) / PLAY_NET_GROUP;
    const PlayNetSide sb = side_of(N, black), sw = side_of(N, white);
    const int same = sb.blob == sw.blob && sb.geo.tag0() == sw.geo.tag0() && sb.geo.tag1() == sw.geo.tag1() ? 1 : 0;
    const Rng rng{env->seed, env->id_base, env->init_rand, env->cur_off, 0};
    const dim3 grid((unsigned)groups), block(64);
    switch (sb.geo.KS) {
#define OTH_PLAY_NET_CASE(K)                                                                                         \
    case K:                                                                                                          \
        launch_k(k_play_net<N, K>, grid, block, 0, st, env->boards, env->meta, env->legal, env->E, env->flags, mode, \
                 sb, sw, same, n_plies, act_in, prot, mask, actions, rewards, dones, plies, env->wdl, env->wdl_vs,   \
                 rng, ctr);                                                                                          \
        break;
        OTH_PLAY_NET_CASE(1)
        OTH_PLAY_NET_CASE(2)
        OTH_PLAY_NET_CASE(3)
        OTH_PLAY_NET_CASE(4)
        OTH_PLAY_NET_CASE(5)
        OTH_PLAY_NET_CASE(6)
        OTH_PLAY_NET_CASE(7)
        OTH_PLAY_NET_CASE(8)
#undef OTH_PLAY_NET_CASE
        default: return fail(OTH_EINVAL, "width must be a multiple of 64 in [64, 512]");
    }
    return after_launch("oth_play_net");
}

template int launch_play_net<OTH_N>(oth_env*, int, const oth_net_policy*, const oth_net_policy*, int, const int32_t*,
                                    const int8_t*, const uint8_t*, int32_t*, int32_t*, uint8_t*, int32_t*, uint64_t,
                                    hipStream_t);

}  // namespace oth_host
