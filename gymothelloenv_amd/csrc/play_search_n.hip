// play_search_n.hip -- k_play_search (oth_play_search, oth_reset_vs_search,
// oth_step_vs_search: the search as a player, play_search.hpp) in a translation
// unit of its own per board size (-DOTH_N=4 .. 16), like search_n.hip.
#include "play_search.hpp"
#include "launch.hpp"

#ifndef OTH_N
#error "compile with -DOTH_N=<board size>"
#endif

using namespace oth;
using namespace oth_dev;

namespace oth_host {

namespace {
PlaySearchSide side_of(const oth_search_policy* p) {
    return PlaySearchSide{p->weights, p->depth, p->mobility_weight, p->terminal_weight, p->endgame_empties,
                          (uint32_t)p->max_nodes};
}
}  // namespace

template <int N>
int launch_play_search(oth_env* env, int mode, const oth_search_policy* black, const oth_search_policy* white,
                       int n_plies, const int32_t* act_in, const int8_t* prot, const uint8_t* mask, int32_t* actions,
                       int32_t* rewards, uint8_t* dones, uint8_t* fb_ply, int32_t* plies, int32_t* fb_cnt,
                       uint64_t ctr, hipStream_t st) {
    const long long groups = ((long long)env->E + SOLVE_GROUP - 1) / SOLVE_GROUP;
    auto k = mode == OTH_PLAY_SEARCH_PLAY ? k_play_search<N, PS_PLAY>
                                          : (mode == OTH_PLAY_SEARCH_STEP_VS ? k_play_search<N, PS_STEP_VS>
                                                                             : k_play_search<N, PS_RESET_VS>);
    const Rng rng{env->seed, env->id_base, env->init_rand, env->cur_off, 0};
    launch_k(k, dim3((unsigned)groups), dim3(SOLVE_BLOCK), 0, st, env->boards, env->meta, env->legal, env->E,
             env->flags, side_of(black), side_of(white), black->weights == white->weights ? 1 : 0, n_plies, act_in,
             prot, mask, actions, rewards, dones, fb_ply, plies, fb_cnt, env->wdl, env->wdl_vs, rng, ctr);
    return after_launch("oth_play_search");
}

template int launch_play_search<OTH_N>(oth_env*, int, const oth_search_policy*, const oth_search_policy*, int,
                                       const int32_t*, const int8_t*, const uint8_t*, int32_t*, int32_t*, uint8_t*,
                                       uint8_t*, int32_t*, int32_t*, uint64_t, hipStream_t);

}  // namespace oth_host
