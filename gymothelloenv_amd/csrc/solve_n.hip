// solve_n.hip -- k_solve (oth_solve: exact endgame values and best moves,
// solve.hpp) in a translation unit of its own per board size (-DOTH_N=4 .. 16),
// like playouts_n.hip.
#include "solve.hpp"
#include "launch.hpp"

#ifndef OTH_N
#error "compile with -DOTH_N=<board size>"
#endif

using namespace oth;
using namespace oth_dev;

namespace oth_host {

template <int N>
int launch_solve(oth_env* env, int max_empties, uint32_t max_nodes, int32_t* value, int32_t* best,
                 int32_t* move_values, uint8_t* status, uint64_t* nodes, hipStream_t st) {
    const long long groups = ((long long)env->E + SOLVE_GROUP - 1) / SOLVE_GROUP;
    launch_k(k_solve<N>, dim3((unsigned)groups), dim3(SOLVE_BLOCK), 0, st, env->boards, env->meta, env->legal, env->E,
             max_empties, max_nodes, value, best, move_values, status, reinterpret_cast<unsigned long long*>(nodes));
    return after_launch("oth_solve");
}

template int launch_solve<OTH_N>(oth_env*, int, uint32_t, int32_t*, int32_t*, int32_t*, uint8_t*, uint64_t*,
                                 hipStream_t);

}  // namespace oth_host
