// launch.hpp -- host side shared by capi.hip and the per-board-size kernel
// translation units (kernels_n.hip): the handle layout, error reporting, and
// the launcher templates, one explicit instantiation per N in kernels_n.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <tuple>
#include <utility>

#include "othello_mi355x.h"
#include "tables.hpp"

struct oth_env {
    int32_t E;
    int32_t n;
    int32_t W;
    uint32_t flags;
    uint64_t seed;
    uint32_t id_base;
    int32_t init_rand;
    int32_t device;
    uint64_t ply;
    uint64_t* boards;
    uint16_t* meta;
    uint64_t* legal;
    unsigned long long* wdl;     // [nslots][4] per-block W/D/L slots by colour (tally)
    unsigned long long* wdl_vs;  // [nslots][4] per-block {protagonist wins, draws, losses} of oth_step_vs
    int32_t nslots;
    // Philox counter offsets (HIP-graph regions, oth_graph_begin/_end):
    // device [OTH_GRAPH_SLOTS][2] = (ply, sample) offsets; slot 0 serves eager
    // launches and stays 0, slot k > 0 belongs to graph region k, whose
    // captured counters start at k << OTH_GRAPH_COUNTER_SHIFT and whose offset
    // moves on by what one replay consumed.
    uint64_t* ctr_slots;
    const uint64_t* cur_off;  // the slot launches read now (slot 0 outside a region)
    int32_t graph_slot;       // open region (0: none)
    uint64_t slots_used;      // bit k: slot k belongs to a captured graph (bit 0, eager, always set)
    uint64_t ply_saved;       // eager ply counter while a region is open
    uint64_t* tables;         // one-word boards: the up rays, then the sel8 table (tables.hpp), read by the
                              // single-ply kernels (rays), k_play_rand and k_playouts (sel8)
    oth_record* rec_host;     // oth_step_sync's record: mapped pinned host memory (allocated on first use)
    oth_record* rec_dev;      // its device address
    uint32_t rec_seq;         // the last record's sequence number
};

namespace oth {
struct NtupleKey;  // ntuple.hpp
}

namespace oth_host {

// error reporting (capi.hip): set the thread's oth_last_error() and return the code
int fail(int code, const char* msg);
int hip_fail(hipError_t err, const char* where);
// the status of the launches since the last after_launch (hipGetLastError too)
int after_launch(const char* what);
void note_launch(hipError_t err);

// Every kernel launch of the C ABI: hipLaunchKernel on the kernel's host stub with
// the arguments converted to the kernel's parameter types, its status kept for
// after_launch.  From C, oth_step costs 3.04 us per call this way against 3.79
// through hipLaunchKernelGGL (same box, tools/launch_cost.hip; profiles/r04/lc/).
template <typename... P, typename... A>
inline void launch_k(void (*k)(P...), dim3 grid, dim3 block, size_t shmem, hipStream_t st, A&&... a) {
    static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
    std::tuple<P...> args{static_cast<P>(std::forward<A>(a))...};
    std::apply([&](auto&... x) {
        void* ptrs[] = {static_cast<void*>(&x)...};
        note_launch(hipLaunchKernel(reinterpret_cast<const void*>(k), grid, block, ptrs, shmem, st));
    }, args);
}

// masked categorical (masked.hip), any board size
int launch_masked(int n_board, int E, const float* logits, long long ld, const uint64_t* legal, const float* uniforms,
                  uint64_t seed, uint32_t id_base, uint64_t counter, const uint64_t* counter_off, int mode,
                  int32_t* actions, float* log_probs, float* entropy, hipStream_t st);

// one set per board size N (kernels_n.hip instantiates them)
template <int N> int launch_reset(oth_env* env, const uint8_t* mask, hipStream_t st);
template <int N>
int launch_step(oth_env* env, const int32_t* actions, int32_t* rewards, uint8_t* dones, uint64_t ply,
                hipStream_t st);
template <int N>
int launch_play(oth_env* env, int policy, int n_plies, int32_t* actions, int32_t* rewards, uint8_t* dones,
                uint64_t ply0, hipStream_t st);
template <int N>
int launch_reset_vs(oth_env* env, int policy, const int8_t* prot, const uint8_t* mask, uint64_t call,
                    hipStream_t st);
template <int N>
int launch_step_vs(oth_env* env, int policy, const int32_t* actions, const int8_t* prot, int32_t* rewards,
                   uint8_t* dones, int32_t* plies, uint64_t call, int obs_layout, int obs_dtype, void* obs,
                   hipStream_t st);
template <int N>
int launch_step_observe(oth_env* env, const int32_t* actions, int32_t* rewards, uint8_t* dones, int layout, int dtype,
                        void* obs, uint64_t ply, hipStream_t st);
// obs: NULL, or the observation (layout, dtype) of the boards after the step (oth_sample_step_observe)
template <int N>
int launch_sample_step(oth_env* env, const float* logits, long long ld, const float* uniforms, uint64_t counter,
                       int mode, int32_t* actions, float* log_probs, float* entropy, int32_t* rewards, uint8_t* dones,
                       uint64_t ply, int obs_layout, int obs_dtype, void* obs, hipStream_t st);
template <int N> int launch_policy_actions(oth_env* env, int policy, int32_t* out, hipStream_t st);
template <int N>
int launch_legal_moves(int n, const uint64_t* mover, const uint64_t* opp, uint64_t* out, hipStream_t st);
template <int N> int launch_observe(oth_env* env, int layout, int dtype, void* out, hipStream_t st);
template <int N> int launch_set_turn(oth_env* env, int turn, const uint8_t* mask, hipStream_t st);
template <int N> int launch_count(oth_env* env, int32_t* out, hipStream_t st);
template <int N> int launch_fill_rays(oth_env* env, hipStream_t st);
template <int N>
int launch_record(oth_env* env, int board, int step, int action, int planes, uint64_t ply, hipStream_t st);
// k_play_rand (one-word boards, random and greedy) and k_play_rand_w (two-word boards,
// random) in play_rand_n.hip, N = 4..11, with its own scheduler flags
template <int N, int POL>
void launch_play_rand(oth_env* env, int n_plies, int32_t* actions, int32_t* rewards, uint8_t* dones, uint64_t ply0,
                      hipStream_t st);

// k_playouts (oth_playouts) in playouts_n.hip, every N, a unit of its own per board size
template <int N>
int launch_playouts(oth_env* env, int mode, int n_playouts, uint64_t seed, uint32_t id_key, uint64_t counter,
                    int32_t* wdl, int32_t* score, int32_t* best, hipStream_t st);

// k_solve (oth_solve) in solve_n.hip, every N, a unit of its own per board size
template <int N>
int launch_solve(oth_env* env, int max_empties, uint32_t max_nodes, int32_t* value, int32_t* best,
                 int32_t* move_values, uint8_t* status, uint64_t* nodes, hipStream_t st);

// k_search (oth_search) in search_n.hip, every N, a unit of its own per board size
template <int N>
int launch_search(oth_env* env, int depth, const int8_t* weights, int mobility, int terminal, uint32_t max_nodes,
                  int32_t* value, int32_t* best, int32_t* move_values, uint8_t* status, uint64_t* nodes,
                  hipStream_t st);

// k_play_search (oth_play_search, oth_reset_vs_search, oth_step_vs_search) in play_search_n.hip, every N, a
// unit of its own per board size.  mode: which of the three; the vs modes pass the opponent as both colours.
// ctr: the first ply's counter (play) or the call's (vs).
enum { OTH_PLAY_SEARCH_PLAY = 0, OTH_PLAY_SEARCH_STEP_VS = 1, OTH_PLAY_SEARCH_RESET_VS = 2 };
template <int N>
int launch_play_search(oth_env* env, int mode, const oth_search_policy* black, const oth_search_policy* white,
                       int n_plies, const int32_t* act_in, const int8_t* prot, const uint8_t* mask, int32_t* actions,
                       int32_t* rewards, uint8_t* dones, uint8_t* fb_ply, int32_t* plies, int32_t* fb_cnt,
                       uint64_t ctr, hipStream_t st);

// k_play_net (oth_play_net, oth_reset_vs_net, oth_step_vs_net) in play_net_n.hip, every N, a unit of its own per
// board size.  mode: which of the three (OTH_PLAY_SEARCH_*); the vs modes pass the opponent as both colours.  ctr:
// the first ply's counter (play) or the call's (vs).  The arguments are checked; the two widths are equal.
template <int N>
int launch_play_net(oth_env* env, int mode, const oth_net_policy* black, const oth_net_policy* white, int n_plies,
                    const int32_t* act_in, const int8_t* prot, const uint8_t* mask, int32_t* actions, int32_t* rewards,
                    uint8_t* dones, int32_t* plies, uint64_t ctr, hipStream_t st);

// k_play_cnet (oth_play_cnet, oth_reset_vs_cnet, oth_step_vs_cnet) in play_cnet_n.hip, every N, a unit of its own
// per board size: launch_play_net's arguments with conv nets.  The arguments are checked; the two channel counts
// are equal.
template <int N>
int launch_play_cnet(oth_env* env, int mode, const oth_cnet_policy* black, const oth_cnet_policy* white, int n_plies,
                     const int32_t* act_in, const int8_t* prot, const uint8_t* mask, int32_t* actions, int32_t* rewards,
                     uint8_t* dones, int32_t* plies, uint64_t ctr, hipStream_t st);

// k_mcts (oth_mcts) in mcts_n.hip, every N, a unit of its own per board size.  The arguments are checked.
template <int N>
int launch_mcts(oth_env* env, const oth_mcts_params* p, void* workspace, int32_t* visits, int32_t* wins2,
                int32_t* best, int32_t* tree_nodes, uint8_t* status, hipStream_t st);
// the 64-bit words of one tree node (mcts.hpp MctsTree::WORDS): three boards of W words, v | w, the links, k | turn
constexpr int mcts_node_words(int n) { return 3 * ((n * n + 63) / 64) + 3; }

// k_puct_begin / k_puct_advance / k_puct_result (oth_puct_*) in puct_n.hip, every N, a unit of its own per
// board size.  The arguments are checked.  A non-NULL obs of the leaves is a second launch (launch_observe on
// the workspace's leaf arrays).
template <int N>
int launch_puct_begin(oth_env* env, const oth_puct_params* p, void* workspace, const oth_puct_leaves* leaves,
                      hipStream_t st);
template <int N>
int launch_puct_advance(oth_env* env, const oth_puct_params* p, void* workspace, const int32_t* priors,
                        const int32_t* values, int more, const oth_puct_leaves* leaves, hipStream_t st);
template <int N>
int launch_puct_result(oth_env* env, const oth_puct_params* p, void* workspace, int32_t* visits, int64_t* value_sums,
                       int32_t* best, int32_t* tree_nodes, uint8_t* status, hipStream_t st);
template <int N>
int launch_puct_pick(oth_env* env, const oth_puct_params* p, void* workspace, const uint8_t* sample, uint64_t seed,
                     uint32_t id_key, uint64_t counter, int32_t* actions, hipStream_t st);
template <int N>
int launch_puct_reroot(oth_env* env, const oth_puct_params* p, void* workspace, const int32_t* actions,
                       const int32_t* root_priors, uint8_t* kept, const oth_puct_leaves* leaves, hipStream_t st);
// k_puct_begin_batch / k_puct_advance_batch / k_puct_reroot_*_batch (oth_puct_*_batch: K leaves a board per
// launch) in puct_n.hip; the observation runs over the extension's E K rows of leaves
template <int N>
int launch_puct_begin_batch(oth_env* env, const oth_puct_params* p, int K, void* workspace,
                            const oth_puct_leaves* leaves, hipStream_t st);
template <int N>
int launch_puct_advance_batch(oth_env* env, const oth_puct_params* p, int K, void* workspace, const int32_t* priors,
                              const int32_t* values, int sim_limit, const oth_puct_leaves* leaves, hipStream_t st);
template <int N>
int launch_puct_reroot_batch(oth_env* env, const oth_puct_params* p, int K, void* workspace, const int32_t* actions,
                             const int32_t* root_priors, uint8_t* kept, int sim_limit, const oth_puct_leaves* leaves,
                             hipStream_t st);
// the 64-bit words of a search's workspace (puct.hpp PuctWs): a tag and a pad, two header words a board, the
// leaves' boards, moves and meta in exchange format, then T nodes a board of three boards of W words and four more
constexpr uint64_t puct_workspace_words(int n, uint64_t E, uint64_t T) {
    return 2u + 2u * E + 3u * (uint64_t)((n * n + 63) / 64) * E + (E + 3u) / 4u +
           E * T * (uint64_t)(3 * ((n * n + 63) / 64) + 4);
}
// ... and of a batch search's (puct.hpp PuctBatchWs): that workspace, then from the next even word two tags, the
// E K rows of leaves in exchange format and a slot word a row
constexpr uint64_t puct_batch_workspace_words(int n, uint64_t E, uint64_t T, uint64_t K) {
    return ((puct_workspace_words(n, E, T) + 1u) & ~1ull) + 2u + 3u * (uint64_t)((n * n + 63) / 64) * E * K +
           (E * K + 3u) / 4u + E * K;
}

// k_replay_* (oth_replay_*: the self-play samples kept, labelled and drawn) and k_symmetry_masks in
// replay_n.hip, every N, a unit of its own per board size.  The arguments are checked.  counts and sample
// are the rank step's two launches first; a non-NULL obs of a batch is one more (launch_observe on the
// batch's exchange-format arrays, the caller's or the workspace's staging rows).
template <int N> int launch_replay_begin(oth_env* env, int H, int B, void* workspace, hipStream_t st);
template <int N>
int launch_replay_append(oth_env* env, int H, int B, void* workspace, const int32_t* visits, const uint8_t* skip,
                         hipStream_t st);
template <int N>
int launch_replay_label(oth_env* env, int H, int B, void* workspace, const int32_t* rewards, const uint8_t* dones,
                        hipStream_t st);
template <int N> int launch_replay_counts(oth_env* env, int H, int B, void* workspace, int64_t* out, hipStream_t st);
// rows_in NULL: oth_replay_sample (augment, seed, id_key, counter); else oth_replay_gather (rows_in, sym_in)
template <int N>
int launch_replay_batch(oth_env* env, int H, int B, void* workspace, int n, const int32_t* rows_in,
                        const uint8_t* sym_in, int augment, uint64_t seed, uint32_t id_key, uint64_t counter,
                        const oth_replay_batch* batch, hipStream_t st);
template <int N>
int launch_symmetry_masks(int n, int planes, const uint8_t* sym, const uint64_t* in, uint64_t* out, hipStream_t st);
// the 64-bit words of a store's workspace (replay.hpp ReplayWs): two tags, two header words a board, the rows'
// state bytes and outcomes, a count word a chunk of 1,024 rows and their prefix, B staging rows in exchange
// format, then the rows' three boards of W words and their N*N visits
constexpr uint64_t replay_workspace_words(int n, uint64_t E, uint64_t H, uint64_t B) {
    return 2u + 2u * E + (E * H + 7u) / 8u + (E * H + 1u) / 2u + (E * H + 1023u) / 1024u +
           ((E * H + 1023u) / 1024u + 2u) / 2u + (B + 3u) / 4u + 3u * (uint64_t)((n * n + 63) / 64) * B +
           3u * (uint64_t)((n * n + 63) / 64) * E * H + (E * H * (uint64_t)(n * n) + 1u) / 2u;
}

// k_net_eval (oth_net_eval: the int8 policy-value network on n_rows >= 1 rows in exchange format) in net.hip, one
// unit for every board size.  The arguments are checked.
int launch_net_eval(int n, const oth_net_params* p, int n_rows, const void* blob, const uint64_t* boards,
                    const uint16_t* meta, const uint64_t* legal, int32_t* priors, int32_t* values, int32_t* logits,
                    hipStream_t st);

// k_cnet_eval (oth_cnet_eval: the int8 residual convolutional network on n_rows >= 1 rows in exchange format) in
// cnet.hip, one unit for every board size.  The arguments are checked.
int launch_cnet_eval(int n, const oth_cnet_params* p, int n_rows, const void* blob, const uint64_t* boards,
                     const uint16_t* meta, const uint64_t* legal, int32_t* priors, int32_t* values, int32_t* logits,
                     hipStream_t st);

// k_puct_noise (oth_puct_noise: Dirichlet root noise mixed into rows of priors) in noise.hip, one unit for every
// board size.  The arguments are checked.
int launch_puct_noise(oth_env* env, int rows_per_board, const uint8_t* kind, const uint64_t* boards,
                      const int32_t* priors_in, int32_t* priors_out, int epsilon, const uint32_t* table, uint64_t seed,
                      uint32_t id_key, uint64_t counter, hipStream_t st);

// k_ntuple_eval (oth_ntuple_eval), k_ntuple_delta + k_ntuple_add (oth_ntuple_update) and k_search_ntuple
// (oth_search_ntuple) in ntuple_n.hip, every N, a unit of its own per board size.  The arguments are checked,
// n_rows >= 1; key: what the plan's header must hold (ntuple.hpp).  mask (oth_ntuple_update_masked): NULL, or
// the rows that learn.
template <int N>
int launch_ntuple_eval(int n_rows, const void* plan, const oth::NtupleKey& key, const int32_t* weights,
                       const uint64_t* boards, const uint16_t* meta, int32_t* values, int64_t* sums, hipStream_t st);
template <int N>
int launch_ntuple_update(int n_rows, const void* plan, const oth::NtupleKey& key, int32_t* weights,
                         const uint64_t* boards, const uint16_t* meta, const int32_t* targets, const uint8_t* mask,
                         int32_t rate, int rate_shift, int32_t* deltas, hipStream_t st);
template <int N>
int launch_search_ntuple(oth_env* env, int depth, const void* plan, const oth::NtupleKey& key, const int32_t* weights,
                         int terminal, uint32_t max_nodes, int32_t* value, int32_t* best, int32_t* move_values,
                         uint8_t* status, uint64_t* nodes, hipStream_t st);

// k_play_ntuple (oth_play_ntuple, oth_reset_vs_ntuple, oth_step_vs_ntuple) in play_ntuple_n.hip, every N, a unit
// of its own per board size: launch_play_search's arguments with n-tuple policies, the keys their plans' headers
// must hold, and td (play mode only; NULL: no rows).  The arguments are checked.
template <int N>
int launch_play_ntuple(oth_env* env, int mode, const oth_ntuple_policy* black, const oth::NtupleKey& key_b,
                       const oth_ntuple_policy* white, const oth::NtupleKey& key_w, int n_plies, const int32_t* act_in,
                       const int8_t* prot, const uint8_t* mask, int32_t* actions, int32_t* rewards, uint8_t* dones,
                       uint8_t* fb_ply, int32_t* plies, int32_t* fb_cnt, const oth_ntuple_td* td, uint64_t ctr,
                       hipStream_t st);

}  // namespace oth_host
