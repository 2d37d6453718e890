// mcts_n.hip -- k_mcts (oth_mcts: a UCT-style tree search per board with
// random-playout leaf evaluation, mcts.hpp) in a translation unit of its own
// per board size (-DOTH_N=4 .. 16), like playouts_n.hip.
#include "mcts.hpp"
#include "launch.hpp"

#ifndef OTH_N
#error "compile with -DOTH_N=<board size>"
#endif

using namespace oth;
using namespace oth_dev;

namespace oth_host {

static_assert(MctsTree<OTH_N>::WORDS == mcts_node_words(OTH_N), "oth_mcts_workspace_bytes' node size");

template <int N>
int launch_mcts(oth_env* env, const oth_mcts_params* p, void* workspace, int32_t* visits, int32_t* wins2,
                int32_t* best, int32_t* tree_nodes, uint8_t* status, hipStream_t st) {
    const int G = MCTS_BLOCK / p->playouts;  // boards a wave
    const long long groups = ((long long)env->E + G - 1) / G;
    const MctsParams mp{p->iterations, p->playouts, p->c_explore, (uint32_t)p->max_tree_nodes,
                        p->seed,       p->counter * 256u, p->id_key};
    launch_k(k_mcts<N>, dim3((unsigned)groups), dim3(MCTS_BLOCK), 0, st, env->boards, env->meta, env->legal, env->E,
             mp, env->id_base, reinterpret_cast<uint64_t*>(workspace), visits, wins2, best, tree_nodes, status);
    return after_launch("oth_mcts");
}

template int launch_mcts<OTH_N>(oth_env*, const oth_mcts_params*, void*, int32_t*, int32_t*, int32_t*, int32_t*,
                                uint8_t*, hipStream_t);

}  // namespace oth_host
