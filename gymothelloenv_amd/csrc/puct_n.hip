// puct_n.hip -- k_puct_begin, k_puct_advance, k_puct_result (oth_puct_begin /
// _advance / _result: a tree search per board whose leaves are evaluated between
// launches, puct.hpp), k_puct_pick and k_puct_reroot_* (oth_puct_pick /
// oth_puct_reroot: the self-play move and the tree carried to the played
// position), and the batch calls' kernels (oth_puct_begin_batch / _advance_batch /
// _reroot_batch: K leaves a board per launch) in a translation unit of its own per board size
// (-DOTH_N=4 .. 16), like mcts_n.hip.
#include "puct.hpp"
#include "launch.hpp"

#ifndef OTH_N
#error "compile with -DOTH_N=<board size>"
#endif

using namespace oth;
using namespace oth_dev;

namespace oth_host {

static_assert(puct_ws_words(OTH_N, 1, OTH_N * OTH_N) == puct_workspace_words(OTH_N, 1, OTH_N * OTH_N) &&
                  puct_ws_words(OTH_N, 70, 4096) == puct_workspace_words(OTH_N, 70, 4096) &&
                  puct_ws_words(OTH_N, 65536, 1 << 24) == puct_workspace_words(OTH_N, 65536, 1 << 24),
              "oth_puct_workspace_bytes' layout");
static_assert(puct_batch_ws_words(OTH_N, 1, OTH_N * OTH_N, 1) == puct_batch_workspace_words(OTH_N, 1, OTH_N * OTH_N, 1) &&
                  puct_batch_ws_words(OTH_N, 70, 4096, 3) == puct_batch_workspace_words(OTH_N, 70, 4096, 3) &&
                  puct_batch_ws_words(OTH_N, 65536, 1 << 24, 64) == puct_batch_workspace_words(OTH_N, 65536, 1 << 24, 64),
              "oth_puct_batch_workspace_bytes' layout");
static_assert(PuctTree<OTH_N>::WORDS == puct_node_words(OTH_N), "the node size");

namespace {

unsigned puct_grid(int E) { return (unsigned)(((long long)E + PUCT_BLOCK - 1) / PUCT_BLOCK); }

// the observation of the leaves: the observation kernels on the workspace's leaf arrays
template <int N>
int puct_observe(oth_env* env, const PuctWs<N>& ws, const oth_puct_leaves* lv, const char* what, hipStream_t st) {
    if (int rc = after_launch(what)) return rc;
    if (!lv || !lv->obs) return OTH_OK;
    oth_env view = *env;  // launch_observe reads the geometry and these three pointers
    view.boards = ws.leaf_boards();
    view.meta = ws.leaf_meta();
    view.legal = ws.leaf_legal();
    return launch_observe<N>(&view, lv->layout, lv->dtype, lv->obs, st);
}

// ... and of a batch call's: the same kernels over the extension's E K rows
template <int N>
int puct_observe_batch(oth_env* env, const PuctBatchWs<N>& bw, const oth_puct_leaves* lv, const char* what,
                       hipStream_t st) {
    if (int rc = after_launch(what)) return rc;
    if (!lv || !lv->obs) return OTH_OK;
    oth_env view = *env;
    view.E = (int32_t)bw.rows();  // (the C ABI has checked that E K fits)
    view.boards = bw.leaf_boards();
    view.meta = bw.leaf_meta();
    view.legal = bw.leaf_legal();
    return launch_observe<N>(&view, lv->layout, lv->dtype, lv->obs, st);
}

PuctLeaves leaves_of(const oth_puct_leaves* lv) {
    if (!lv) return PuctLeaves{nullptr, nullptr, nullptr, nullptr};
    return PuctLeaves{lv->kind, lv->boards, lv->meta, lv->legal};
}

}  // namespace

template <int N>
int launch_puct_begin(oth_env* env, const oth_puct_params* p, void* workspace, const oth_puct_leaves* lv,
                      hipStream_t st) {
    const PuctWs<N> ws{reinterpret_cast<uint64_t*>(workspace), (uint32_t)env->E, (uint32_t)p->max_tree_nodes};
    launch_k(k_puct_begin<N>, dim3(puct_grid(env->E)), dim3(PUCT_BLOCK), 0, st, env->boards, env->meta, env->legal,
             env->E, ws.T, ws.base, leaves_of(lv));
    return puct_observe<N>(env, ws, lv, "oth_puct_begin", st);
}

template <int N>
int launch_puct_advance(oth_env* env, const oth_puct_params* p, void* workspace, const int32_t* priors,
                        const int32_t* values, int more, const oth_puct_leaves* lv, hipStream_t st) {
    const PuctWs<N> ws{reinterpret_cast<uint64_t*>(workspace), (uint32_t)env->E, (uint32_t)p->max_tree_nodes};
    launch_k(k_puct_advance<N>, dim3(puct_grid(env->E)), dim3(PUCT_BLOCK), 0, st, env->E, ws.T, p->c_puct, ws.base,
             priors, values, more, leaves_of(lv));
    return puct_observe<N>(env, ws, lv, "oth_puct_advance", st);
}

template <int N>
int launch_puct_result(oth_env* env, const oth_puct_params* p, void* workspace, int32_t* visits, int64_t* value_sums,
                       int32_t* best, int32_t* tree_nodes, uint8_t* status, hipStream_t st) {
    launch_k(k_puct_result<N>, dim3(puct_grid(env->E)), dim3(PUCT_BLOCK), 0, st, env->E,
             (uint32_t)p->max_tree_nodes, reinterpret_cast<uint64_t*>(workspace), visits, value_sums, best, tree_nodes,
             status);
    return after_launch("oth_puct_result");
}

template <int N>
int launch_puct_pick(oth_env* env, const oth_puct_params* p, void* workspace, const uint8_t* sample, uint64_t seed,
                     uint32_t id_key, uint64_t counter, int32_t* actions, hipStream_t st) {
    launch_k(k_puct_pick<N>, dim3(puct_grid(env->E)), dim3(PUCT_BLOCK), 0, st, env->E, (uint32_t)p->max_tree_nodes,
             reinterpret_cast<uint64_t*>(workspace), sample, seed, id_key + env->id_base, counter, actions);
    return after_launch("oth_puct_pick");
}

template <int N>
int launch_puct_reroot(oth_env* env, const oth_puct_params* p, void* workspace, const int32_t* actions,
                       const int32_t* root_priors, uint8_t* kept, const oth_puct_leaves* lv, hipStream_t st) {
    const PuctWs<N> ws{reinterpret_cast<uint64_t*>(workspace), (uint32_t)env->E, (uint32_t)p->max_tree_nodes};
    const dim3 grid(puct_grid(env->E)), block(PUCT_BLOCK);
#if OTH_PUCT_REROOT_LANE
    launch_k(k_puct_reroot_lane<N>, grid, block, 0, st, env->boards, env->meta, env->legal, env->E, ws.T, p->c_puct,
             ws.base, actions, root_priors, kept, leaves_of(lv));
#else
    launch_k(k_puct_reroot_classify<N>, grid, block, 0, st, env->boards, env->meta, env->legal, env->E, ws.T, ws.base,
             actions, leaves_of(lv));
    launch_k(k_puct_reroot_sweep<N>, dim3((unsigned)env->E), dim3(64), 0, st, env->E, ws.T, ws.base);
    launch_k(k_puct_reroot_finish<N>, grid, block, 0, st, env->E, ws.T, p->c_puct, ws.base, root_priors, kept,
             leaves_of(lv));
#endif
    return puct_observe<N>(env, ws, lv, "oth_puct_reroot", st);
}

template <int N>
int launch_puct_begin_batch(oth_env* env, const oth_puct_params* p, int K, void* workspace, const oth_puct_leaves* lv,
                            hipStream_t st) {
    const PuctBatchWs<N> bw{PuctWs<N>{reinterpret_cast<uint64_t*>(workspace), (uint32_t)env->E,
                                      (uint32_t)p->max_tree_nodes}, (uint32_t)K};
    launch_k(k_puct_begin_batch<N>, dim3(puct_grid(env->E)), dim3(PUCT_BLOCK), 0, st, env->boards, env->meta,
             env->legal, env->E, bw.plain.T, bw.K, bw.plain.base, leaves_of(lv));
    return puct_observe_batch<N>(env, bw, lv, "oth_puct_begin_batch", st);
}

template <int N>
int launch_puct_advance_batch(oth_env* env, const oth_puct_params* p, int K, void* workspace, const int32_t* priors,
                              const int32_t* values, int sim_limit, const oth_puct_leaves* lv, hipStream_t st) {
    const PuctBatchWs<N> bw{PuctWs<N>{reinterpret_cast<uint64_t*>(workspace), (uint32_t)env->E,
                                      (uint32_t)p->max_tree_nodes}, (uint32_t)K};
    launch_k(k_puct_advance_batch<N>, dim3(puct_grid(env->E)), dim3(PUCT_BLOCK), 0, st, env->E, bw.plain.T, bw.K,
             p->c_puct, bw.plain.base, priors, values, (uint32_t)sim_limit, leaves_of(lv));
    return puct_observe_batch<N>(env, bw, lv, "oth_puct_advance_batch", st);
}

template <int N>
int launch_puct_reroot_batch(oth_env* env, const oth_puct_params* p, int K, void* workspace, const int32_t* actions,
                             const int32_t* root_priors, uint8_t* kept, int sim_limit, const oth_puct_leaves* lv,
                             hipStream_t st) {
    const PuctBatchWs<N> bw{PuctWs<N>{reinterpret_cast<uint64_t*>(workspace), (uint32_t)env->E,
                                      (uint32_t)p->max_tree_nodes}, (uint32_t)K};
    const dim3 grid(puct_grid(env->E)), block(PUCT_BLOCK);
    launch_k(k_puct_reroot_classify_batch<N>, grid, block, 0, st, env->boards, env->meta, env->legal, env->E,
             bw.plain.T, bw.K, bw.plain.base, actions);
    launch_k(k_puct_reroot_sweep_batch<N>, dim3((unsigned)env->E), dim3(64), 0, st, env->E, bw.plain.T, bw.K,
             bw.plain.base);
    launch_k(k_puct_reroot_finish_batch<N>, grid, block, 0, st, env->E, bw.plain.T, bw.K, p->c_puct, bw.plain.base,
             root_priors, kept, (uint32_t)sim_limit, leaves_of(lv));
    return puct_observe_batch<N>(env, bw, lv, "oth_puct_reroot_batch", st);
}

template int launch_puct_begin<OTH_N>(oth_env*, const oth_puct_params*, void*, const oth_puct_leaves*, hipStream_t);
template int launch_puct_advance<OTH_N>(oth_env*, const oth_puct_params*, void*, const int32_t*, const int32_t*, int,
                                        const oth_puct_leaves*, hipStream_t);
template int launch_puct_result<OTH_N>(oth_env*, const oth_puct_params*, void*, int32_t*, int64_t*, int32_t*, int32_t*,
                                       uint8_t*, hipStream_t);
template int launch_puct_pick<OTH_N>(oth_env*, const oth_puct_params*, void*, const uint8_t*, uint64_t, uint32_t, uint64_t,
                                     int32_t*, hipStream_t);
template int launch_puct_reroot<OTH_N>(oth_env*, const oth_puct_params*, void*, const int32_t*, const int32_t*, uint8_t*,
                                       const oth_puct_leaves*, hipStream_t);
template int launch_puct_begin_batch<OTH_N>(oth_env*, const oth_puct_params*, int, void*, const oth_puct_leaves*,
                                            hipStream_t);
template int launch_puct_advance_batch<OTH_N>(oth_env*, const oth_puct_params*, int, void*, const int32_t*,
                                              const int32_t*, int, const oth_puct_leaves*, hipStream_t);
template int launch_puct_reroot_batch<OTH_N>(oth_env*, const oth_puct_params*, int, void*, const int32_t*,
                                             const int32_t*, uint8_t*, int, const oth_puct_leaves*, hipStream_t);

}  // namespace oth_host
