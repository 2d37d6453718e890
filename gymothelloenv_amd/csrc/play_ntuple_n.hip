// play_ntuple_n.hip -- k_play_ntuple (oth_play_ntuple, oth_reset_vs_ntuple, oth_step_vs_ntuple: the n-tuple
// network as a player, play_ntuple.hpp) in a translation unit of its own per board size (-DOTH_N=4 .. 16), like
// play_search_n.hip.
#include "play_ntuple.hpp"
#include "launch.hpp"

#ifndef OTH_N
#error "compile with -DOTH_N=<board size>"
#endif

using namespace oth;
using namespace oth_dev;

static_assert(NTUPLE_EXPLORE_ONE == OTH_NTUPLE_EXPLORE_ONE, "the header's");

namespace oth_host {

namespace {
PlayNtupleSide side_of(const oth_ntuple_policy* p) {
    return PlayNtupleSide{static_cast<const uint32_t*>(p->plan), p->weights, p->depth, p->terminal_weight,
                          p->endgame_empties, p->explore, (uint32_t)p->max_nodes};
}
bool same_key(const NtupleKey& a, const NtupleKey& b) {
    return a.n == b.n && a.tuples == b.tuples && a.shift == b.shift && a.n_weights == b.n_weights && a.hash == b.hash;
}
}  // namespace

template <int N>
int launch_play_ntuple(oth_env* env, int mode, const oth_ntuple_policy* black, const NtupleKey& key_b,
                       const oth_ntuple_policy* white, const NtupleKey& key_w, int n_plies, const int32_t* act_in,
                       const int8_t* prot, const uint8_t* mask, int32_t* actions, int32_t* rewards, uint8_t* dones,
                       uint8_t* fb_ply, int32_t* plies, int32_t* fb_cnt, const oth_ntuple_td* td, uint64_t ctr,
                       hipStream_t st) {
    const long long groups = ((long long)env->E + SOLVE_GROUP - 1) / SOLVE_GROUP;
    auto k = mode == OTH_PLAY_SEARCH_PLAY ? k_play_ntuple<N, PS_PLAY>
                                          : (mode == OTH_PLAY_SEARCH_STEP_VS ? k_play_ntuple<N, PS_STEP_VS>
                                                                             : k_play_ntuple<N, PS_RESET_VS>);
    const Rng rng{env->seed, env->id_base, env->init_rand, env->cur_off, 0};
    const PlayNtupleTd rows = td ? PlayNtupleTd{td->boards, td->meta, td->targets, td->learn}
                                 : PlayNtupleTd{nullptr, nullptr, nullptr, nullptr};
    launch_k(k, dim3((unsigned)groups), dim3(SOLVE_BLOCK), 0, st, env->boards, env->meta, env->legal, env->E,
             env->flags, side_of(black), side_of(white), key_b, key_w,
             black->plan == white->plan && same_key(key_b, key_w) ? 1 : 0, n_plies, act_in, prot, mask, actions,
             rewards, dones, fb_ply, plies, fb_cnt, env->wdl, env->wdl_vs, rows, rng, ctr);
    return after_launch("oth_play_ntuple");
}

template int launch_play_ntuple<OTH_N>(oth_env*, int, const oth_ntuple_policy*, const NtupleKey&,
                                       const oth_ntuple_policy*, const NtupleKey&, int, const int32_t*, const int8_t*,
                                       const uint8_t*, int32_t*, int32_t*, uint8_t*, uint8_t*, int32_t*, int32_t*,
                                       const oth_ntuple_td*, uint64_t, hipStream_t);

}  // namespace oth_host
