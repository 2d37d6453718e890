// search_n.hip -- k_search (oth_search: depth-limited alpha-beta over weighted
// squares and mobility, search.hpp) in a translation unit of its own per board
// size (-DOTH_N=4 .. 16), like solve_n.hip.
#include "search.hpp"
#include "launch.hpp"

#ifndef OTH_N
#error "compile with -DOTH_N=<board size>"
#endif

using namespace oth;
using namespace oth_dev;

namespace oth_host {

template <int N>
int launch_search(oth_env* env, int depth, const int8_t* weights, int mobility, int terminal, uint32_t max_nodes,
                  int32_t* value, int32_t* best, int32_t* move_values, uint8_t* status, uint64_t* nodes,
                  hipStream_t st) {
    const long long groups = ((long long)env->E + SOLVE_GROUP - 1) / SOLVE_GROUP;
    launch_k(k_search<N>, dim3((unsigned)groups), dim3(SOLVE_BLOCK), 0, st, env->boards, env->meta, env->legal, env->E,
             depth, weights, mobility, terminal, max_nodes, value, best, move_values, status,
             reinterpret_cast<unsigned long long*>(nodes));
    return after_launch("oth_search");
}

template int launch_search<OTH_N>(oth_env*, int, const int8_t*, int, int, uint32_t, int32_t*, int32_t*, int32_t*,
                                  uint8_t*, uint64_t*, hipStream_t);

}  // namespace oth_host
