// capi.hip -- the C ABI declared in include/othello_mi355x.h: argument checks,
// handle lifetime, error reporting and dispatch on the board size to the
// per-N launchers (kernels_n.hip).
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include <new>
#include <string>
#include <type_traits>

#include "launch.hpp"
#include "net.hpp"
#include "cnet.hpp"
#include "ntuple.hpp"

using namespace oth;
using namespace oth_host;

namespace oth_host {

thread_local std::string g_last_error;

int fail(int code, const char* msg) {
    g_last_error = msg;
    return code;
}

int hip_fail(hipError_t err, const char* where) {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", where, hipGetErrorString(err));
    g_last_error = buf;
    return OTH_EHIP;
}

namespace {
thread_local hipError_t g_launch_err = hipSuccess;  // the first failed launch since after_launch
}

void note_launch(hipError_t err) {
    if (err != hipSuccess && g_launch_err == hipSuccess) g_launch_err = err;
}

int after_launch(const char* what) {
    hipError_t err = g_launch_err;
    g_launch_err = hipSuccess;
    const hipError_t last = hipGetLastError();  // (and clears HIP's own sticky status)
    if (err == hipSuccess) err = last;
    if (err != hipSuccess) return hip_fail(err, what);
    return OTH_OK;
}

}  // namespace oth_host

namespace {

#define OTH_HIP(call)                                         \
    do {                                                      \
        hipError_t err_ = (call);                             \
        if (err_ != hipSuccess) return hip_fail(err_, #call); \
    } while (0)

template <typename Fn>
int with_n(int n, Fn&& fn) {
    switch (n) {
        case 4: return fn(std::integral_constant<int, 4>{});
        case 5: return fn(std::integral_constant<int, 5>{});
        case 6: return fn(std::integral_constant<int, 6>{});
        case 7: return fn(std::integral_constant<int, 7>{});
        case 8: return fn(std::integral_constant<int, 8>{});
        case 9: return fn(std::integral_constant<int, 9>{});
        case 10: return fn(std::integral_constant<int, 10>{});
        case 11: return fn(std::integral_constant<int, 11>{});
        case 12: return fn(std::integral_constant<int, 12>{});
        case 13: return fn(std::integral_constant<int, 13>{});
        case 14: return fn(std::integral_constant<int, 14>{});
        case 15: return fn(std::integral_constant<int, 15>{});
        case 16: return fn(std::integral_constant<int, 16>{});
        default: return fail(OTH_EINVAL, "board_size must be in [4, 16]");
    }
}

int use_device(const oth_env* env) {
    int cur = -1;
    OTH_HIP(hipGetDevice(&cur));
    if (cur != env->device) OTH_HIP(hipSetDevice(env->device));
    return OTH_OK;
}

#define OTH_CHECK_ENV(env)                                    \
    do {                                                      \
        if (!(env)) return fail(OTH_EINVAL, "NULL oth_env");  \
        int rc_ = use_device(env);                            \
        if (rc_) return rc_;                                  \
    } while (0)

// oth_counts: sum the per-block slots into out[3] (int64); optionally zero them.
__global__ __launch_bounds__(256) void k_reduce_wdl(unsigned long long* __restrict__ wdl, int nslots,
                                                   int64_t* __restrict__ out, int reset) {
    __shared__ unsigned long long acc[256][3];
    unsigned long long b = 0, d = 0, w = 0;
    for (int i = threadIdx.x; i < nslots; i += 256) {
        b += wdl[4 * (size_t)i];
        d += wdl[4 * (size_t)i + 1];
        w += wdl[4 * (size_t)i + 2];
        if (reset) {
            wdl[4 * (size_t)i] = 0;
            wdl[4 * (size_t)i + 1] = 0;
            wdl[4 * (size_t)i + 2] = 0;
        }
    }
    acc[threadIdx.x][0] = b;
    acc[threadIdx.x][1] = d;
    acc[threadIdx.x][2] = w;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            acc[threadIdx.x][0] += acc[threadIdx.x + s][0];
            acc[threadIdx.x][1] += acc[threadIdx.x + s][1];
            acc[threadIdx.x][2] += acc[threadIdx.x + s][2];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) out[threadIdx.x] = (int64_t)acc[0][threadIdx.x];
}

// The leaves of one MaxiMin(d) search from a position with e empty squares:
// `root` moves at the root, then at most min(b, e - j) at level j, since every
// level places a disc (simple_policies.py:138) and a full board ends the game
// (:117-121); b = max(2, N*N / 6) moves per position (8x8 middle games: ~10).
double search_leaves(int d, int e, double root, double b) {
    double leaves = 1.0;
    for (int j = 0; j < d && j < e; ++j) {
        const double moves = j == 0 ? root : (b < e - j ? b : (double)(e - j));
        if (moves <= 0.0) break;  // no move: the search stops here (:120)
        leaves *= moves;
    }
    return leaves;
}

enum MaximinCall { MM_POLICY, MM_STEP_VS, MM_RESET_VS };

// MaxiMin searches of depth >= 3 are refused above OTH_MAXIMIN_LEAF_BUDGET
// estimated leaves per call.  First E x b^d x `searches` (the searches one board
// runs in the call: plies of oth_step_policy, opponent replies of the _vs calls);
// above the budget, the boards are read and each live board's search bounded by
// its own position (search_leaves: its empty squares, and its possible_moves at
// the root of a policy call), so late-game boards are searched at any depth the
// budget allows -- one 8x8 board with 10 empty squares at depth 10 is <= 10!
// leaves, where the position-blind estimate says 1.9e10.
int maximin_budget(const oth_env* env, int policy, double searches, MaximinCall call, hipStream_t st) {
    if (policy < OTH_POLICY_MAXIMIN(3) || policy > OTH_POLICY_LAST) return OTH_OK;
    const int d = policy - OTH_POLICY_MAXIMIN1 + 1, nn = env->n * env->n;
    const double b = nn / 6.0 > 2.0 ? nn / 6.0 : 2.0;
    double leaves = (double)env->E * searches;
    for (int i = 0; i < d; ++i) leaves *= b;
    if (leaves <= OTH_MAXIMIN_LEAF_BUDGET) return OTH_OK;
    const char* why = "";
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (call == MM_RESET_VS) {
        why = " (reset_vs searches from the start position)";
    } else if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        why = " (during a stream capture the boards cannot be read for a position-aware estimate)";
    } else {
        const size_t E = (size_t)env->E, W = (size_t)env->W;
        uint64_t* bd = new (std::nothrow) uint64_t[E * 3 * W];
        uint16_t* meta = new (std::nothrow) uint16_t[E];
        if (!bd || !meta) {
            delete[] bd;
            delete[] meta;
            return fail(OTH_ENOMEM, "maximin budget: host allocation failed");
        }
        uint64_t* lg = bd + E * 2 * W;
        hipError_t err = hipMemcpyAsync(bd, env->boards, E * 2 * W * 8, hipMemcpyDeviceToHost, st);
        if (err == hipSuccess) err = hipMemcpyAsync(lg, env->legal, E * W * 8, hipMemcpyDeviceToHost, st);
        if (err == hipSuccess) err = hipMemcpyAsync(meta, env->meta, E * 2, hipMemcpyDeviceToHost, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        if (err != hipSuccess) {
            delete[] bd;
            delete[] meta;
            return hip_fail(err, "maximin budget: reading the boards");
        }
        // with auto-reset a board that ends is searched again from the start position
        const bool resets = (env->flags & OTH_AUTO_RESET) != 0;
        leaves = 0.0;
        for (size_t i = 0; i < E; ++i) {
            const bool done = (meta[i] & 2) != 0;
            if (done && !resets) continue;  // terminated: no search
            int discs = 0, moves = 0;
            for (size_t w = 0; w < 2 * W; ++w) discs += __builtin_popcountll(bd[i * 2 * W + w]);
            for (size_t w = 0; w < W; ++w) moves += __builtin_popcountll(lg[i * W + w]);
            const int e = nn - discs, later = resets && nn - 4 > e ? nn - 4 : e;
            const double rest = search_leaves(d, later, b < later ? b : (double)later, b);
            if (call == MM_POLICY && !done)  // the first search from this position, later plies from <= `later` empties
                leaves += search_leaves(d, e, (double)moves, b) + (searches - 1.0) * rest;
            else  // the opponent's replies after the protagonist's move (or searches after a reset)
                leaves += searches * rest;
        }
        delete[] bd;
        delete[] meta;
        if (leaves <= OTH_MAXIMIN_LEAF_BUDGET) return OTH_OK;
        why = " (bounded by each board's empty squares)";
    }
    char msg[320];
    snprintf(msg, sizeof(msg), "MaxiMin depth %d over %d boards of %dx%d (x%.0f searches) is ~%.1e leaves%s, above the "
             "budget of %.1e per call: split the boards over calls or search shallower", d, env->E, env->n, env->n,
             searches, leaves, why, (double)OTH_MAXIMIN_LEAF_BUDGET);
    return fail(OTH_EINVAL, msg);
}

}  // namespace

extern "C" {

const char* oth_last_error(void) { return g_last_error.c_str(); }

#ifndef OTH_SRC_HASH
#define OTH_SRC_HASH "0000000000000000000000000000000000000000000000000000000000000000"
#endif
// build.py passes the SHA-256 of the sources and flags; the loader compares it
// with the tree's sources (gymothelloenv_amd/build.py: embedded_hash)
const char* oth_version(void) { return "othello_mi355x 0.2 (gfx950) oth-src-sha256:" OTH_SRC_HASH; }

int oth_create(int32_t n_envs, int32_t board_size, uint32_t flags, uint64_t seed, uint32_t env_id_base,
               int32_t initial_rand_steps, int32_t device, oth_env** out) {
    if (!out) return fail(OTH_EINVAL, "out is NULL");
    *out = nullptr;
    if (n_envs <= 0) return fail(OTH_EINVAL, "n_envs must be > 0");
    const int n = board_size < 4 ? 4 : board_size;  // othello.py:230
    if (n > 16) return fail(OTH_EINVAL, "board_size must be <= 16");
    if (initial_rand_steps < 0 || initial_rand_steps > 255)
        return fail(OTH_EINVAL, "initial_rand_steps must be in [0, 255]");
    if (flags & ~7u) return fail(OTH_EINVAL, "unknown flag bits");
    OTH_HIP(hipSetDevice(device));
    oth_env* env = new (std::nothrow) oth_env();
    if (!env) return fail(OTH_ENOMEM, "host allocation failed");
    env->E = n_envs;
    env->n = n;
    env->W = (n * n + 63) / 64;
    env->flags = flags;
    env->seed = seed;
    env->id_base = env_id_base;
    env->init_rand = initial_rand_steps;
    env->device = device;
    env->ply = 0;
    const size_t E = (size_t)n_envs, W = (size_t)env->W;
    hipError_t err = hipMalloc((void**)&env->boards, E * 2 * W * sizeof(uint64_t));
    if (err == hipSuccess) err = hipMalloc((void**)&env->meta, ((E * sizeof(uint16_t) + 15) / 16) * 16);
    if (err == hipSuccess) err = hipMalloc((void**)&env->legal, E * W * sizeof(uint64_t));
    // one W/D/L slot per wave of the widest single-ply grid (k_sample_step4: 4 lanes per board) -- also
    // more than the per-block slots of every multi-ply launch
    env->nslots = (int32_t)((4 * (int64_t)E + 63) / 64);
    const size_t slot_bytes = (size_t)env->nslots * 4 * sizeof(unsigned long long);
    if (err == hipSuccess) err = hipMalloc((void**)&env->wdl, slot_bytes);
    if (err == hipSuccess) err = hipMemset(env->wdl, 0, slot_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&env->wdl_vs, slot_bytes);
    if (err == hipSuccess) err = hipMemset(env->wdl_vs, 0, slot_bytes);
    const size_t ctr_bytes = (size_t)OTH_GRAPH_SLOTS * 2 * sizeof(uint64_t);
    if (err == hipSuccess) err = hipMalloc((void**)&env->ctr_slots, ctr_bytes);
    if (err == hipSuccess) err = hipMemset(env->ctr_slots, 0, ctr_bytes);
    if (err == hipSuccess && env->W == 1) err = hipMalloc((void**)&env->tables, TABLE_WORDS * sizeof(uint64_t));
    env->cur_off = env->ctr_slots;
    env->graph_slot = 0;
    env->slots_used = 1;
    if (err != hipSuccess) {
        oth_destroy(env);
        return hip_fail(err, "oth_create: allocation");
    }
    int rc = with_n(n, [&](auto NC) { return launch_fill_rays<decltype(NC)::value>(env, nullptr); });
    if (rc == OTH_OK) rc = oth_reset(env, nullptr, nullptr);
    if (rc == OTH_OK) {
        err = hipStreamSynchronize(nullptr);
        if (err != hipSuccess) rc = hip_fail(err, "oth_create: reset");
    }
    if (rc != OTH_OK) {
        oth_destroy(env);
        return rc;
    }
    *out = env;
    return OTH_OK;
}

int oth_destroy(oth_env* env) {
    if (!env) return OTH_OK;
    (void)hipSetDevice(env->device);
    if (env->boards) (void)hipFree(env->boards);
    if (env->meta) (void)hipFree(env->meta);
    if (env->legal) (void)hipFree(env->legal);
    if (env->wdl) (void)hipFree(env->wdl);
    if (env->wdl_vs) (void)hipFree(env->wdl_vs);
    if (env->ctr_slots) (void)hipFree(env->ctr_slots);
    if (env->tables) (void)hipFree(env->tables);
    if (env->rec_host) (void)hipHostFree(env->rec_host);
    delete env;
    return OTH_OK;
}

int oth_reset(oth_env* env, const uint8_t* mask, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    return with_n(env->n, [&](auto NC) { return launch_reset<decltype(NC)::value>(env, mask, (hipStream_t)stream); });
}

int oth_step(oth_env* env, const int32_t* actions, int32_t* rewards, uint8_t* dones, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (!actions) return fail(OTH_EINVAL, "actions is NULL");
    const uint64_t ply = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_step<decltype(NC)::value>(env, actions, rewards, dones, ply, (hipStream_t)stream);
    });
}

int oth_step_observe(oth_env* env, const int32_t* actions, int32_t* rewards, uint8_t* dones, int32_t layout,
                     int32_t dtype, void* obs, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (!actions || !obs) return fail(OTH_EINVAL, "actions / obs is NULL");
    if (layout < OTH_OBS_BOARD || layout > OTH_OBS_LEGAL) return fail(OTH_EINVAL, "unknown layout");
    if (dtype < OTH_I8 || dtype > OTH_BF16) return fail(OTH_EINVAL, "unknown dtype");
    const uint64_t ply = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_step_observe<decltype(NC)::value>(env, actions, rewards, dones, layout, dtype, obs, ply,
                                                        (hipStream_t)stream);
    });
}

int oth_step_sync(oth_env* env, int32_t board, int32_t step, int32_t action, int32_t layout, const oth_record** out,
                  oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (!out) return fail(OTH_EINVAL, "out is NULL");
    if (board < 0 || board >= env->E) return fail(OTH_EINVAL, "board out of range");
    if (layout != OTH_OBS_BOARD && layout != OTH_OBS_BOARD_LEGAL)
        return fail(OTH_EINVAL, "layout must be OTH_OBS_BOARD or OTH_OBS_BOARD_LEGAL");
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    OTH_HIP(hipStreamIsCapturing((hipStream_t)stream, &cap));
    if (cap != hipStreamCaptureStatusNone)  // it waits for its record: never inside a graph capture
        return fail(OTH_EINVAL, "oth_step_sync waits for its result and cannot run during a stream capture");
    if (!env->rec_host) {  // mapped, coherent pinned host memory: the kernel's stores land in it directly
        void* h = nullptr;
        OTH_HIP(hipHostMalloc(&h, sizeof(oth_record), hipHostMallocMapped | hipHostMallocCoherent));
        memset(h, 0, sizeof(oth_record));
        void* d = nullptr;
        const hipError_t err = hipHostGetDevicePointer(&d, h, 0);
        if (err != hipSuccess) {
            (void)hipHostFree(h);
            return hip_fail(err, "oth_step_sync: hipHostGetDevicePointer");
        }
        env->rec_host = static_cast<oth_record*>(h);
        env->rec_dev = static_cast<oth_record*>(d);
        env->rec_seq = 0;
    }
    const uint32_t seq = ++env->rec_seq;
    const uint64_t ply = (step & 1) ? env->ply++ : env->ply;
    const int rc = with_n(env->n, [&](auto NC) {
        return launch_record<decltype(NC)::value>(env, board, step & (1 | OTH_RECORD_GREEDY), action,
                                                  layout == OTH_OBS_BOARD_LEGAL ? 2 : 1, ply, (hipStream_t)stream);
    });
    if (rc) return rc;
    // wait for the sequence number (the kernel writes it last, behind a system-scope
    // fence): no runtime synchronisation on the path; after a bounded spin the
    // stream is synchronised instead, which also reports a failed kernel
    const volatile uint32_t* sp = &env->rec_host->seq;
    for (int i = 0; i < (1 << 22); ++i) {
        if (*sp == seq) {
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            *out = env->rec_host;
            return OTH_OK;
        }
        __builtin_ia32_pause();
    }
    OTH_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (*sp != seq) return fail(OTH_EHIP, "oth_step_sync: the record did not arrive");
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    *out = env->rec_host;
    return OTH_OK;
}

int oth_step_policy(oth_env* env, int32_t policy, int32_t n_plies, int32_t* actions, int32_t* rewards,
                    uint8_t* dones, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (n_plies < 0) return fail(OTH_EINVAL, "n_plies must be >= 0");
    if (policy < OTH_POLICY_RANDOM || policy > OTH_POLICY_LAST) return fail(OTH_EINVAL, "unknown policy");
    if (n_plies == 0) return OTH_OK;
    if (int rc = maximin_budget(env, policy, (double)n_plies, MM_POLICY, (hipStream_t)stream)) return rc;
    const uint64_t ply0 = env->ply;
    env->ply += (uint64_t)n_plies;
    return with_n(env->n, [&](auto NC) {
        return launch_play<decltype(NC)::value>(env, policy, n_plies, actions, rewards, dones, ply0,
                                                (hipStream_t)stream);
    });
}

int oth_playouts(oth_env* env, int32_t mode, int32_t n_playouts, uint64_t seed, uint32_t id_key, uint64_t counter,
                 int32_t* wdl, int32_t* score, int32_t* best, oth_stream_t stream) {
    // the argument checks come before the device is touched
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (!wdl) return fail(OTH_EINVAL, "wdl is NULL");
    if (mode != OTH_PLAYOUT_ROOT && mode != OTH_PLAYOUT_MOVES) return fail(OTH_EINVAL, "unknown playout mode");
    if (n_playouts < 1 || n_playouts > OTH_PLAYOUTS_MAX)
        return fail(OTH_EINVAL, "n_playouts must be in [1, 65536]");
    if (best && mode == OTH_PLAYOUT_ROOT) return fail(OTH_EINVAL, "best is per move: NULL in OTH_PLAYOUT_ROOT mode");
    if (counter >> 56) return fail(OTH_EINVAL, "counter must be below 2^56");
    const int64_t per_env = (int64_t)n_playouts * (mode == OTH_PLAYOUT_MOVES ? env->n * env->n : 1);
    if ((int64_t)env->E * per_env > 0x7fffffffll)
        return fail(OTH_EINVAL, "more than 2^31 - 1 playouts in one call: split the boards or the playouts");
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_playouts<decltype(NC)::value>(env, mode, n_playouts, seed, id_key, counter, wdl, score, best,
                                                    (hipStream_t)stream);
    });
}

int oth_solve(oth_env* env, int32_t max_empties, uint64_t max_nodes, int32_t* value, int32_t* best,
              int32_t* move_values, uint8_t* status, uint64_t* nodes, oth_stream_t stream) {
    // the argument checks come before the handle is read
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (!value) return fail(OTH_EINVAL, "value is NULL");
    if (max_empties < 1 || max_empties > OTH_SOLVE_MAX_EMPTIES)
        return fail(OTH_EINVAL, "max_empties must be in [1, 14]");
    if (max_nodes < 1 || max_nodes > 0xffffffffull) return fail(OTH_EINVAL, "max_nodes must be in [1, 2^32 - 1]");
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_solve<decltype(NC)::value>(env, max_empties, (uint32_t)max_nodes, value, best, move_values,
                                                 status, nodes, (hipStream_t)stream);
    });
}

int oth_mcts_workspace_bytes(int32_t board_size, int32_t n_envs, int32_t max_tree_nodes, uint64_t* bytes) {
    if (!bytes) return fail(OTH_EINVAL, "bytes is NULL");
    if (board_size < 4 || board_size > 16) return fail(OTH_EINVAL, "board_size must be in [4, 16]");
    if (n_envs < 1) return fail(OTH_EINVAL, "n_envs must be >= 1");
    if (max_tree_nodes < board_size * board_size || max_tree_nodes > OTH_MCTS_MAX_TREE_NODES)
        return fail(OTH_EINVAL, "max_tree_nodes must be in [N*N, 2^24]");
    *bytes = (uint64_t)n_envs * (uint64_t)max_tree_nodes * (uint64_t)mcts_node_words(board_size) * 8u;
    return OTH_OK;
}

int oth_mcts(oth_env* env, const oth_mcts_params* p, void* workspace, uint64_t workspace_bytes, int32_t* visits,
             int32_t* wins2, int32_t* best, int32_t* tree_nodes, uint8_t* status, oth_stream_t stream) {
    // what needs no handle to decide comes first; all of it before the device is touched
    if (!p) return fail(OTH_EINVAL, "params is NULL");
    if (!workspace) return fail(OTH_EINVAL, "workspace is NULL");
    if (!visits) return fail(OTH_EINVAL, "visits is NULL");
    if (p->iterations < 1 || p->iterations > OTH_MCTS_MAX_ITERATIONS)
        return fail(OTH_EINVAL, "iterations must be in [1, 65535]");
    if (p->playouts < 1 || p->playouts > OTH_MCTS_MAX_PLAYOUTS) return fail(OTH_EINVAL, "playouts must be in [1, 64]");
    if (p->c_explore < 0 || p->c_explore > OTH_MCTS_MAX_C) return fail(OTH_EINVAL, "c_explore must be in [0, 65535]");
    if (p->max_tree_nodes < 16 || p->max_tree_nodes > OTH_MCTS_MAX_TREE_NODES)
        return fail(OTH_EINVAL, "max_tree_nodes must be in [N*N, 2^24]");
    if (p->counter >> 56) return fail(OTH_EINVAL, "counter must be below 2^56");
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return fail(OTH_EINVAL, "workspace must be 8-byte aligned");
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    uint64_t need = 0;
    if (int rc = oth_mcts_workspace_bytes(env->n, env->E, p->max_tree_nodes, &need)) return rc;
    if (workspace_bytes < need)
        return fail(OTH_EINVAL, "workspace_bytes is below what oth_mcts_workspace_bytes reports");
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_mcts<decltype(NC)::value>(env, p, workspace, visits, wins2, best, tree_nodes, status,
                                                (hipStream_t)stream);
    });
}

int oth_puct_workspace_bytes(int32_t board_size, int32_t n_envs, int32_t max_tree_nodes, uint64_t* bytes) {
    if (!bytes) return fail(OTH_EINVAL, "bytes is NULL");
    if (board_size < 4 || board_size > 16) return fail(OTH_EINVAL, "board_size must be in [4, 16]");
    if (n_envs < 1) return fail(OTH_EINVAL, "n_envs must be >= 1");
    if (max_tree_nodes < board_size * board_size || max_tree_nodes > OTH_PUCT_MAX_TREE_NODES)
        return fail(OTH_EINVAL, "max_tree_nodes must be in [N*N, 2^24]");
    *bytes = puct_workspace_words(board_size, (uint64_t)n_envs, (uint64_t)max_tree_nodes) * 8u;
    return OTH_OK;
}

namespace {

// What the three oth_puct calls share, in oth_mcts' order: what needs no handle to decide first, all of it
// before the device is touched.
int puct_check(const oth_env* env, const oth_puct_params* p, const void* workspace, uint64_t workspace_bytes,
               const oth_puct_leaves* leaves) {
    if (!p) return fail(OTH_EINVAL, "params is NULL");
    if (!workspace) return fail(OTH_EINVAL, "workspace is NULL");
    if (p->c_puct < 0 || p->c_puct > OTH_PUCT_MAX_C) return fail(OTH_EINVAL, "c_puct must be in [0, 65535]");
    if (p->max_tree_nodes < 16 || p->max_tree_nodes > OTH_PUCT_MAX_TREE_NODES)
        return fail(OTH_EINVAL, "max_tree_nodes must be in [N*N, 2^24]");
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return fail(OTH_EINVAL, "workspace must be 8-byte aligned");
    if (leaves && leaves->obs) {
        if (leaves->layout < OTH_OBS_BOARD || leaves->layout > OTH_OBS_LEGAL)
            return fail(OTH_EINVAL, "unknown layout of the leaves' obs");
        if (leaves->dtype < OTH_I8 || leaves->dtype > OTH_BF16)
            return fail(OTH_EINVAL, "unknown dtype of the leaves' obs");
    }
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    uint64_t need = 0;
    if (int rc = oth_puct_workspace_bytes(env->n, env->E, p->max_tree_nodes, &need)) return rc;
    if (workspace_bytes < need)
        return fail(OTH_EINVAL, "workspace_bytes is below what oth_puct_workspace_bytes reports");
    return OTH_OK;
}

}  // namespace

int oth_puct_begin(oth_env* env, const oth_puct_params* p, void* workspace, uint64_t workspace_bytes,
                   const oth_puct_leaves* leaves, oth_stream_t stream) {
    if (int rc = puct_check(env, p, workspace, workspace_bytes, leaves)) return rc;
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_puct_begin<decltype(NC)::value>(env, p, workspace, leaves, (hipStream_t)stream);
    });
}

int oth_puct_advance(oth_env* env, const oth_puct_params* p, void* workspace, uint64_t workspace_bytes,
                     const int32_t* priors, const int32_t* values, int32_t more, const oth_puct_leaves* leaves,
                     oth_stream_t stream) {
    if (!priors) return fail(OTH_EINVAL, "priors is NULL");
    if (!values) return fail(OTH_EINVAL, "values is NULL");
    if (int rc = puct_check(env, p, workspace, workspace_bytes, leaves)) return rc;
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_puct_advance<decltype(NC)::value>(env, p, workspace, priors, values, more, leaves,
                                                        (hipStream_t)stream);
    });
}

int oth_puct_result(oth_env* env, const oth_puct_params* p, void* workspace, uint64_t workspace_bytes,
                    int32_t* visits, int64_t* value_sums, int32_t* best, int32_t* tree_nodes, uint8_t* status,
                    oth_stream_t stream) {
    if (!visits) return fail(OTH_EINVAL, "visits is NULL");
    if (int rc = puct_check(env, p, workspace, workspace_bytes, nullptr)) return rc;
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_puct_result<decltype(NC)::value>(env, p, workspace, visits, value_sums, best, tree_nodes, status,
                                                       (hipStream_t)stream);
    });
}

int oth_puct_pick(oth_env* env, const oth_puct_params* p, void* workspace, uint64_t workspace_bytes,
                  const uint8_t* sample, uint64_t seed, uint32_t id_key, uint64_t counter, int32_t* actions,
                  oth_stream_t stream) {
    if (!actions) return fail(OTH_EINVAL, "actions is NULL");
    if (int rc = puct_check(env, p, workspace, workspace_bytes, nullptr)) return rc;
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_puct_pick<decltype(NC)::value>(env, p, workspace, sample, seed, id_key, counter, actions,
                                                     (hipStream_t)stream);
    });
}

int oth_puct_reroot(oth_env* env, const oth_puct_params* p, void* workspace, uint64_t workspace_bytes,
                    const int32_t* actions, const int32_t* root_priors, uint8_t* kept, const oth_puct_leaves* leaves,
                    oth_stream_t stream) {
    if (!actions) return fail(OTH_EINVAL, "actions is NULL");
    if (int rc = puct_check(env, p, workspace, workspace_bytes, leaves)) return rc;
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_puct_reroot<decltype(NC)::value>(env, p, workspace, actions, root_priors, kept, leaves,
                                                       (hipStream_t)stream);
    });
}

int oth_puct_batch_workspace_bytes(int32_t board_size, int32_t n_envs, int32_t max_tree_nodes, int32_t K,
                                   uint64_t* bytes) {
    uint64_t plain = 0;
    if (!bytes) return fail(OTH_EINVAL, "bytes is NULL");
    if (int rc = oth_puct_workspace_bytes(board_size, n_envs, max_tree_nodes, &plain)) return rc;
    if (K < 1 || K > OTH_PUCT_MAX_LEAVES) return fail(OTH_EINVAL, "K must be in [1, 64]");
    *bytes = puct_batch_workspace_words(board_size, (uint64_t)n_envs, (uint64_t)max_tree_nodes, (uint64_t)K) * 8u;
    return OTH_OK;
}

namespace {

// What the three batch calls share beyond puct_check, in its order: K and sim_limit need no handle
int puct_batch_check(const oth_env* env, const oth_puct_params* p, int32_t K, const void* workspace,
                     uint64_t workspace_bytes, const oth_puct_leaves* leaves, int32_t sim_limit) {
    if (K < 1 || K > OTH_PUCT_MAX_LEAVES) return fail(OTH_EINVAL, "K must be in [1, 64]");
    if (sim_limit < 0 || sim_limit > OTH_PUCT_MAX_SIMS) return fail(OTH_EINVAL, "sim_limit must be in [0, 2^24 - 1]");
    if (int rc = puct_check(env, p, workspace, workspace_bytes, leaves)) return rc;
    if ((int64_t)env->E * K > 0x7fffffffll) return fail(OTH_EINVAL, "more than 2^31 - 1 rows of leaves: n_envs K");
    uint64_t need = 0;
    if (int rc = oth_puct_batch_workspace_bytes(env->n, env->E, p->max_tree_nodes, K, &need)) return rc;
    if (workspace_bytes < need)
        return fail(OTH_EINVAL, "workspace_bytes is below what oth_puct_batch_workspace_bytes reports");
    return OTH_OK;
}

}  // namespace

int oth_puct_begin_batch(oth_env* env, const oth_puct_params* p, int32_t K, void* workspace, uint64_t workspace_bytes,
                         const oth_puct_leaves* leaves, oth_stream_t stream) {
    if (int rc = puct_batch_check(env, p, K, workspace, workspace_bytes, leaves, 0)) return rc;
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_puct_begin_batch<decltype(NC)::value>(env, p, K, workspace, leaves, (hipStream_t)stream);
    });
}

int oth_puct_advance_batch(oth_env* env, const oth_puct_params* p, int32_t K, void* workspace,
                           uint64_t workspace_bytes, const int32_t* priors, const int32_t* values, int32_t sim_limit,
                           const oth_puct_leaves* leaves, oth_stream_t stream) {
    if (!priors) return fail(OTH_EINVAL, "priors is NULL");
    if (!values) return fail(OTH_EINVAL, "values is NULL");
    if (int rc = puct_batch_check(env, p, K, workspace, workspace_bytes, leaves, sim_limit)) return rc;
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_puct_advance_batch<decltype(NC)::value>(env, p, K, workspace, priors, values, sim_limit, leaves,
                                                              (hipStream_t)stream);
    });
}

int oth_puct_reroot_batch(oth_env* env, const oth_puct_params* p, int32_t K, void* workspace, uint64_t workspace_bytes,
                          const int32_t* actions, const int32_t* root_priors, uint8_t* kept, int32_t sim_limit,
                          const oth_puct_leaves* leaves, oth_stream_t stream) {
    if (!actions) return fail(OTH_EINVAL, "actions is NULL");
    if (int rc = puct_batch_check(env, p, K, workspace, workspace_bytes, leaves, sim_limit)) return rc;
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_puct_reroot_batch<decltype(NC)::value>(env, p, K, workspace, actions, root_priors, kept,
                                                             sim_limit, leaves, (hipStream_t)stream);
    });
}

int oth_replay_workspace_bytes(int32_t board_size, int32_t n_envs, int32_t horizon, int32_t max_batch,
                               uint64_t* bytes) {
    if (!bytes) return fail(OTH_EINVAL, "bytes is NULL");
    if (board_size < 4 || board_size > 16) return fail(OTH_EINVAL, "board_size must be in [4, 16]");
    if (n_envs < 1) return fail(OTH_EINVAL, "n_envs must be >= 1");
    if (horizon < 1 || horizon > OTH_REPLAY_MAX_HORIZON) return fail(OTH_EINVAL, "horizon must be in [1, 65536]");
    if (max_batch < 1 || max_batch > OTH_REPLAY_MAX_BATCH) return fail(OTH_EINVAL, "max_batch must be in [1, 2^20]");
    if ((uint64_t)n_envs * (uint64_t)horizon > (uint64_t)OTH_REPLAY_MAX_ROWS)
        return fail(OTH_EINVAL, "n_envs * horizon must be at most 2^24");
    *bytes = replay_workspace_words(board_size, (uint64_t)n_envs, (uint64_t)horizon, (uint64_t)max_batch) * 8u;
    return OTH_OK;
}

namespace {

// What the oth_replay calls share, in the puct calls' order: what needs no handle to decide first, all of it
// before the device is touched.  batch: the call's oth_replay_batch, or NULL; n: its rows (1 without one).
int replay_check(const oth_env* env, int32_t horizon, int32_t max_batch, const void* workspace,
                 uint64_t workspace_bytes, const oth_replay_batch* batch, int32_t n) {
    if (!workspace) return fail(OTH_EINVAL, "workspace is NULL");
    if (horizon < 1 || horizon > OTH_REPLAY_MAX_HORIZON) return fail(OTH_EINVAL, "horizon must be in [1, 65536]");
    if (max_batch < 1 || max_batch > OTH_REPLAY_MAX_BATCH) return fail(OTH_EINVAL, "max_batch must be in [1, 2^20]");
    if (n < 1 || n > OTH_REPLAY_MAX_BATCH) return fail(OTH_EINVAL, "n must be in [1, max_batch]");
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return fail(OTH_EINVAL, "workspace must be 8-byte aligned");
    if (batch && batch->obs) {
        if (batch->layout < OTH_OBS_BOARD || batch->layout > OTH_OBS_LEGAL)
            return fail(OTH_EINVAL, "unknown layout of the batch's obs");
        if (batch->dtype < OTH_I8 || batch->dtype > OTH_BF16)
            return fail(OTH_EINVAL, "unknown dtype of the batch's obs");
    }
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    uint64_t need = 0;
    if (int rc = oth_replay_workspace_bytes(env->n, env->E, horizon, max_batch, &need)) return rc;
    if (workspace_bytes < need)
        return fail(OTH_EINVAL, "workspace_bytes is below what oth_replay_workspace_bytes reports");
    if (n > max_batch) return fail(OTH_EINVAL, "n must be in [1, max_batch]");
    return OTH_OK;
}

}  // namespace

int oth_replay_begin(oth_env* env, int32_t horizon, int32_t max_batch, void* workspace, uint64_t workspace_bytes,
                     oth_stream_t stream) {
    if (int rc = replay_check(env, horizon, max_batch, workspace, workspace_bytes, nullptr, 1)) return rc;
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_replay_begin<decltype(NC)::value>(env, horizon, max_batch, workspace, (hipStream_t)stream);
    });
}

int oth_replay_append(oth_env* env, int32_t horizon, int32_t max_batch, void* workspace, uint64_t workspace_bytes,
                      const int32_t* visits, const uint8_t* skip, oth_stream_t stream) {
    if (!visits) return fail(OTH_EINVAL, "visits is NULL");
    if (int rc = replay_check(env, horizon, max_batch, workspace, workspace_bytes, nullptr, 1)) return rc;
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_replay_append<decltype(NC)::value>(env, horizon, max_batch, workspace, visits, skip,
                                                         (hipStream_t)stream);
    });
}

int oth_replay_label(oth_env* env, int32_t horizon, int32_t max_batch, void* workspace, uint64_t workspace_bytes,
                     const int32_t* rewards, const uint8_t* dones, oth_stream_t stream) {
    if (!rewards) return fail(OTH_EINVAL, "rewards is NULL");
    if (!dones) return fail(OTH_EINVAL, "dones is NULL");
    if (int rc = replay_check(env, horizon, max_batch, workspace, workspace_bytes, nullptr, 1)) return rc;
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_replay_label<decltype(NC)::value>(env, horizon, max_batch, workspace, rewards, dones,
                                                        (hipStream_t)stream);
    });
}

int oth_replay_counts(oth_env* env, int32_t horizon, int32_t max_batch, void* workspace, uint64_t workspace_bytes,
                      int64_t* out, oth_stream_t stream) {
    if (!out) return fail(OTH_EINVAL, "out is NULL");
    if (int rc = replay_check(env, horizon, max_batch, workspace, workspace_bytes, nullptr, 1)) return rc;
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_replay_counts<decltype(NC)::value>(env, horizon, max_batch, workspace, out, (hipStream_t)stream);
    });
}

int oth_replay_gather(oth_env* env, int32_t horizon, int32_t max_batch, void* workspace, uint64_t workspace_bytes,
                      int32_t n, const int32_t* rows_in, const uint8_t* sym_in, const oth_replay_batch* batch,
                      oth_stream_t stream) {
    if (!rows_in) return fail(OTH_EINVAL, "rows_in is NULL");
    if (!batch) return fail(OTH_EINVAL, "batch is NULL");
    if (int rc = replay_check(env, horizon, max_batch, workspace, workspace_bytes, batch, n)) return rc;
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_replay_batch<decltype(NC)::value>(env, horizon, max_batch, workspace, n, rows_in, sym_in, 0, 0, 0,
                                                        0, batch, (hipStream_t)stream);
    });
}

int oth_replay_sample(oth_env* env, int32_t horizon, int32_t max_batch, void* workspace, uint64_t workspace_bytes,
                      int32_t n, int32_t augment, uint64_t seed, uint32_t id_key, uint64_t counter,
                      const oth_replay_batch* batch, oth_stream_t stream) {
    if (!batch) return fail(OTH_EINVAL, "batch is NULL");
    if (int rc = replay_check(env, horizon, max_batch, workspace, workspace_bytes, batch, n)) return rc;
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_replay_batch<decltype(NC)::value>(env, horizon, max_batch, workspace, n, nullptr, nullptr,
                                                        augment != 0, seed, id_key, counter, batch,
                                                        (hipStream_t)stream);
    });
}

int oth_symmetry_masks(int32_t board_size, int32_t n, int32_t planes, const uint8_t* sym, const uint64_t* in,
                       uint64_t* out, oth_stream_t stream) {
    if (!sym || !in || !out) return fail(OTH_EINVAL, "sym, in or out is NULL");
    if (in == out) return fail(OTH_EINVAL, "in and out must be different arrays");
    if (n < 1 || planes < 1 || (int64_t)n * planes > INT32_MAX)
        return fail(OTH_EINVAL, "n and planes must be >= 1 and n * planes at most 2^31 - 1");
    if (board_size < 4 || board_size > 16) return fail(OTH_EINVAL, "board_size must be in [4, 16]");
    return with_n(board_size, [&](auto NC) {
        return launch_symmetry_masks<decltype(NC)::value>(n, planes, sym, in, out, (hipStream_t)stream);
    });
}

namespace {
// oth_net_params as net.hpp's NetParams, checked: what every oth_net call does first
int net_params(int32_t board_size, const oth_net_params* params, NetParams* out) {
    if (!params) return fail(OTH_EINVAL, "params is NULL");
    out->layers = params->layers;
    out->width = params->width;
    for (int l = 0; l < 4; ++l) out->shift[l] = params->shift[l];
    out->policy_shift = params->policy_shift;
    out->value_shift = params->value_shift;
    if (const char* why = net_check(board_size, out)) return fail(OTH_EINVAL, why);
    return OTH_OK;
}
}  // namespace

int oth_net_blob_bytes(int32_t board_size, const oth_net_params* params, uint64_t* bytes) {
    if (!bytes) return fail(OTH_EINVAL, "bytes is NULL");
    NetParams np;
    if (int rc = net_params(board_size, params, &np)) return rc;
    *bytes = net_geo(board_size, np).bytes();
    return OTH_OK;
}

int oth_net_pack(int32_t board_size, const oth_net_params* params, const int8_t* w, const int32_t* b, void* blob,
                 uint64_t blob_bytes) {
    if (!w || !b || !blob) return fail(OTH_EINVAL, "w, b or blob is NULL");
    NetParams np;
    if (int rc = net_params(board_size, params, &np)) return rc;
    if (reinterpret_cast<uintptr_t>(blob) & 15u) return fail(OTH_EINVAL, "blob must be 16-byte aligned");
    if (blob_bytes < net_geo(board_size, np).bytes())
        return fail(OTH_EINVAL, "blob_bytes is below what oth_net_blob_bytes reports");
    if (const char* why = net_pack(board_size, np, w, b, reinterpret_cast<uint8_t*>(blob))) return fail(OTH_EINVAL, why);
    return OTH_OK;
}

int oth_net_eval(int32_t board_size, int32_t n_rows, const oth_net_params* params, const void* blob,
                 uint64_t blob_bytes, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal,
                 int32_t* priors, int32_t* values, int32_t* logits, oth_stream_t stream) {
    if (!blob) return fail(OTH_EINVAL, "blob is NULL");
    if (!boards || !meta || !legal) return fail(OTH_EINVAL, "boards, meta or legal is NULL");
    if (!priors || !values) return fail(OTH_EINVAL, "priors or values is NULL");
    NetParams np;
    if (int rc = net_params(board_size, params, &np)) return rc;
    if (n_rows < 0 || n_rows > OTH_NET_MAX_ROWS) return fail(OTH_EINVAL, "n_rows must be in [0, 2^24]");
    if (reinterpret_cast<uintptr_t>(blob) & 15u) return fail(OTH_EINVAL, "blob must be 16-byte aligned");
    if (blob_bytes < net_geo(board_size, np).bytes())
        return fail(OTH_EINVAL, "blob_bytes is below what oth_net_blob_bytes reports");
    if (n_rows == 0) return OTH_OK;
    return launch_net_eval(board_size, params, n_rows, blob, boards, meta, legal, priors, values, logits,
                           (hipStream_t)stream);
}

namespace {
// oth_cnet_params as cnet.hpp's CnetParams, checked: what every oth_cnet call does first
int cnet_params(int32_t board_size, const oth_cnet_params* params, CnetParams* out) {
    if (!params) return fail(OTH_EINVAL, "params is NULL");
    out->channels = params->channels;
    out->blocks = params->blocks;
    out->shift_stem = params->shift_stem;
    for (int l = 0; l < 16; ++l) out->shift[l] = params->shift[l];
    out->shift_head = params->shift_head;
    out->policy_shift = params->policy_shift;
    out->value_shift = params->value_shift;
    if (const char* why = cnet_check(board_size, out)) return fail(OTH_EINVAL, why);
    return OTH_OK;
}
}  // namespace

int oth_cnet_blob_bytes(int32_t board_size, const oth_cnet_params* params, uint64_t* bytes) {
    if (!bytes) return fail(OTH_EINVAL, "bytes is NULL");
    CnetParams cp;
    if (int rc = cnet_params(board_size, params, &cp)) return rc;
    *bytes = cnet_geo(board_size, cp).bytes();
    return OTH_OK;
}

int oth_cnet_pack(int32_t board_size, const oth_cnet_params* params, const int8_t* w, const int32_t* b, void* blob,
                  uint64_t blob_bytes) {
    if (!w || !b || !blob) return fail(OTH_EINVAL, "w, b or blob is NULL");
    CnetParams cp;
    if (int rc = cnet_params(board_size, params, &cp)) return rc;
    if (reinterpret_cast<uintptr_t>(blob) & 15u) return fail(OTH_EINVAL, "blob must be 16-byte aligned");
    if (blob_bytes < cnet_geo(board_size, cp).bytes())
        return fail(OTH_EINVAL, "blob_bytes is below what oth_cnet_blob_bytes reports");
    if (const char* why = cnet_pack(board_size, cp, w, b, reinterpret_cast<uint8_t*>(blob))) return fail(OTH_EINVAL, why);
    return OTH_OK;
}

int oth_cnet_eval(int32_t board_size, int32_t n_rows, const oth_cnet_params* params, const void* blob,
                  uint64_t blob_bytes, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal,
                  int32_t* priors, int32_t* values, int32_t* logits, oth_stream_t stream) {
    if (!blob) return fail(OTH_EINVAL, "blob is NULL");
    if (!boards || !meta || !legal) return fail(OTH_EINVAL, "boards, meta or legal is NULL");
    if (!priors || !values) return fail(OTH_EINVAL, "priors or values is NULL");
    CnetParams cp;
    if (int rc = cnet_params(board_size, params, &cp)) return rc;
    if (n_rows < 0 || n_rows > OTH_NET_MAX_ROWS) return fail(OTH_EINVAL, "n_rows must be in [0, 2^24]");
    if (reinterpret_cast<uintptr_t>(blob) & 15u) return fail(OTH_EINVAL, "blob must be 16-byte aligned");
    if (blob_bytes < cnet_geo(board_size, cp).bytes())
        return fail(OTH_EINVAL, "blob_bytes is below what oth_cnet_blob_bytes reports");
    if (n_rows == 0) return OTH_OK;
    return launch_cnet_eval(board_size, params, n_rows, blob, boards, meta, legal, priors, values, logits,
                            (hipStream_t)stream);
}

int oth_puct_noise(oth_env* env, int32_t rows_per_board, const uint8_t* kind, const uint64_t* boards,
                   const int32_t* priors_in, int32_t* priors_out, int32_t epsilon, const uint32_t* table, uint64_t seed,
                   uint32_t id_key, uint64_t counter, oth_stream_t stream) {
    // what needs no handle to decide first, all of it before the device is touched
    if (!priors_in || !priors_out) return fail(OTH_EINVAL, "priors_in or priors_out is NULL");
    if (!table) return fail(OTH_EINVAL, "table is NULL");
    if ((kind == nullptr) != (boards == nullptr)) return fail(OTH_EINVAL, "kind and boards go together: both or neither");
    if (rows_per_board < 1 || rows_per_board > OTH_PUCT_MAX_LEAVES)
        return fail(OTH_EINVAL, "rows_per_board must be in [1, 64]");
    if (epsilon < 0 || epsilon > 256) return fail(OTH_EINVAL, "epsilon must be in [0, 256]");
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if ((int64_t)env->E * rows_per_board > INT32_MAX) return fail(OTH_EINVAL, "n_envs * rows_per_board must fit 31 bits");
    if (int rc = use_device(env)) return rc;
    return launch_puct_noise(env, rows_per_board, kind, boards, priors_in, priors_out, epsilon, table, seed, id_key,
                             counter, (hipStream_t)stream);
}

int oth_search(oth_env* env, int32_t depth, const int8_t* weights, int32_t mobility_weight, int32_t terminal_weight,
               uint64_t max_nodes, int32_t* value, int32_t* best, int32_t* move_values, uint8_t* status,
               uint64_t* nodes, oth_stream_t stream) {
    // the argument checks come before the handle is read
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (!value) return fail(OTH_EINVAL, "value is NULL");
    if (!weights) return fail(OTH_EINVAL, "weights is NULL");
    if (depth < 1 || depth > OTH_SEARCH_MAX_DEPTH) return fail(OTH_EINVAL, "depth must be in [1, 14]");
    if (mobility_weight < -127 || mobility_weight > 127)
        return fail(OTH_EINVAL, "mobility_weight must be in [-127, 127]");
    if (terminal_weight < 1 || terminal_weight > 32767)
        return fail(OTH_EINVAL, "terminal_weight must be in [1, 32767]");
    if (max_nodes < 1 || max_nodes > 0xffffffffull) return fail(OTH_EINVAL, "max_nodes must be in [1, 2^32 - 1]");
    if (int rc = use_device(env)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_search<decltype(NC)::value>(env, depth, weights, mobility_weight, terminal_weight,
                                                  (uint32_t)max_nodes, value, best, move_values, status, nodes,
                                                  (hipStream_t)stream);
    });
}

}  // extern "C"

namespace {
static_assert(sizeof(oth_ntuple_params) == sizeof(NtupleParams), "ntuple.hpp's NtupleParams is the header's struct");

// oth_ntuple_params as ntuple.hpp's NtupleParams, checked: what every oth_ntuple call does first
int ntuple_params(int32_t board_size, const oth_ntuple_params* params, NtupleParams* out) {
    if (!params) return fail(OTH_EINVAL, "params is NULL");
    memcpy(out, params, sizeof(*out));
    if (const char* why = ntuple_check(board_size, out)) return fail(OTH_EINVAL, why);
    return OTH_OK;
}

// the plan and the weights of a device call, against the parameters
int ntuple_device_args(const NtupleParams& np, const void* plan, uint64_t plan_bytes, const void* weights,
                       uint64_t weight_count) {
    if (!plan) return fail(OTH_EINVAL, "plan is NULL");
    if (!weights) return fail(OTH_EINVAL, "weights is NULL");
    if (reinterpret_cast<uintptr_t>(plan) & 7u) return fail(OTH_EINVAL, "plan must be 8-byte aligned");
    if (plan_bytes < ntuple_plan_bytes(np)) return fail(OTH_EINVAL, "plan_bytes is below what oth_ntuple_plan_bytes reports");
    if (weight_count < (uint64_t)ntuple_n_weights(np) + 1u)
        return fail(OTH_EINVAL, "weight_count is below what oth_ntuple_weight_count reports");
    return OTH_OK;
}
}  // namespace

extern "C" {

int oth_ntuple_weight_count(int32_t board_size, const oth_ntuple_params* params, uint64_t* count) {
    if (!count) return fail(OTH_EINVAL, "count is NULL");
    NtupleParams np;
    if (int rc = ntuple_params(board_size, params, &np)) return rc;
    *count = (uint64_t)ntuple_n_weights(np) + 1u;
    return OTH_OK;
}

int oth_ntuple_plan_bytes(int32_t board_size, const oth_ntuple_params* params, uint64_t* bytes) {
    if (!bytes) return fail(OTH_EINVAL, "bytes is NULL");
    NtupleParams np;
    if (int rc = ntuple_params(board_size, params, &np)) return rc;
    *bytes = ntuple_plan_bytes(np);
    return OTH_OK;
}

int oth_ntuple_plan(int32_t board_size, const oth_ntuple_params* params, void* plan, uint64_t plan_bytes) {
    if (!plan) return fail(OTH_EINVAL, "plan is NULL");
    NtupleParams np;
    if (int rc = ntuple_params(board_size, params, &np)) return rc;
    if (reinterpret_cast<uintptr_t>(plan) & 7u) return fail(OTH_EINVAL, "plan must be 8-byte aligned");
    if (plan_bytes < ntuple_plan_bytes(np)) return fail(OTH_EINVAL, "plan_bytes is below what oth_ntuple_plan_bytes reports");
    ntuple_plan(board_size, np, static_cast<uint32_t*>(plan));
    return OTH_OK;
}

int oth_ntuple_eval(int32_t board_size, int32_t n_rows, const oth_ntuple_params* params, const void* plan,
                    uint64_t plan_bytes, const int32_t* weights, uint64_t weight_count, const uint64_t* boards,
                    const uint16_t* meta, int32_t* values, int64_t* sums, oth_stream_t stream) {
    if (!boards || !meta) return fail(OTH_EINVAL, "boards or meta is NULL");
    if (!values) return fail(OTH_EINVAL, "values is NULL");
    NtupleParams np;
    if (int rc = ntuple_params(board_size, params, &np)) return rc;
    if (int rc = ntuple_device_args(np, plan, plan_bytes, weights, weight_count)) return rc;
    if (n_rows < 0 || n_rows > OTH_NTUPLE_MAX_ROWS) return fail(OTH_EINVAL, "n_rows must be in [0, 2^24]");
    if (n_rows == 0) return OTH_OK;
    const NtupleKey key = ntuple_key(board_size, np);
    return with_n(board_size, [&](auto NC) {
        return launch_ntuple_eval<decltype(NC)::value>(n_rows, plan, key, weights, boards, meta, values, sums,
                                                       (hipStream_t)stream);
    });
}

int oth_ntuple_update(int32_t board_size, int32_t n_rows, const oth_ntuple_params* params, const void* plan,
                      uint64_t plan_bytes, int32_t* weights, uint64_t weight_count, const uint64_t* boards,
                      const uint16_t* meta, const int32_t* targets, int32_t rate, int32_t rate_shift, int32_t* deltas,
                      oth_stream_t stream) {
    return oth_ntuple_update_masked(board_size, n_rows, params, plan, plan_bytes, weights, weight_count, boards, meta,
                                    targets, nullptr, rate, rate_shift, deltas, stream);
}

int oth_ntuple_update_masked(int32_t board_size, int32_t n_rows, const oth_ntuple_params* params, const void* plan,
                             uint64_t plan_bytes, int32_t* weights, uint64_t weight_count, const uint64_t* boards,
                             const uint16_t* meta, const int32_t* targets, const uint8_t* mask, int32_t rate,
                             int32_t rate_shift, int32_t* deltas, oth_stream_t stream) {
    if (!boards || !meta) return fail(OTH_EINVAL, "boards or meta is NULL");
    if (!targets) return fail(OTH_EINVAL, "targets is NULL");
    if (!deltas) return fail(OTH_EINVAL, "deltas is NULL");
    NtupleParams np;
    if (int rc = ntuple_params(board_size, params, &np)) return rc;
    if (int rc = ntuple_device_args(np, plan, plan_bytes, weights, weight_count)) return rc;
    if (n_rows < 0 || n_rows > OTH_NTUPLE_MAX_ROWS) return fail(OTH_EINVAL, "n_rows must be in [0, 2^24]");
    if (rate < 0 || rate > OTH_NTUPLE_MAX_RATE) return fail(OTH_EINVAL, "rate must be in [0, 2^24]");
    if (rate_shift < 0 || rate_shift > OTH_NTUPLE_MAX_RATE_SHIFT) return fail(OTH_EINVAL, "rate_shift must be in [0, 40]");
    if (n_rows == 0) return OTH_OK;
    const NtupleKey key = ntuple_key(board_size, np);
    return with_n(board_size, [&](auto NC) {
        return launch_ntuple_update<decltype(NC)::value>(n_rows, plan, key, weights, boards, meta, targets, mask, rate,
                                                         rate_shift, deltas, (hipStream_t)stream);
    });
}

int oth_search_ntuple(oth_env* env, int32_t depth, const oth_ntuple_params* params, const void* plan,
                      uint64_t plan_bytes, const int32_t* weights, uint64_t weight_count, int32_t terminal_weight,
                      uint64_t max_nodes, int32_t* value, int32_t* best, int32_t* move_values, uint8_t* status,
                      uint64_t* nodes, oth_stream_t stream) {
    // the argument checks come before the handle's device is touched
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (!value) return fail(OTH_EINVAL, "value is NULL");
    NtupleParams np;
    if (int rc = ntuple_params(env->n, params, &np)) return rc;
    if (int rc = ntuple_device_args(np, plan, plan_bytes, weights, weight_count)) return rc;
    if (depth < 1 || depth > OTH_SEARCH_MAX_DEPTH) return fail(OTH_EINVAL, "depth must be in [1, 14]");
    if (terminal_weight < 1 || terminal_weight > 32767)
        return fail(OTH_EINVAL, "terminal_weight must be in [1, 32767]");
    if (max_nodes < 1 || max_nodes > 0xffffffffull) return fail(OTH_EINVAL, "max_nodes must be in [1, 2^32 - 1]");
    if (int rc = use_device(env)) return rc;
    const NtupleKey key = ntuple_key(env->n, np);
    return with_n(env->n, [&](auto NC) {
        return launch_search_ntuple<decltype(NC)::value>(env, depth, plan, key, weights, terminal_weight,
                                                         (uint32_t)max_nodes, value, best, move_values, status, nodes,
                                                         (hipStream_t)stream);
    });
}

}  // extern "C"

namespace {
// an oth_search_policy's ranges (oth_search's); who: the argument's name for the message
int check_search_policy(const oth_search_policy* p, const char* who) {
    char msg[160];
    const char* why = nullptr;
    if (!p) why = "is NULL";
    else if (!p->weights) why = "has NULL weights";
    else if (p->depth < 1 || p->depth > OTH_SEARCH_MAX_DEPTH) why = "depth must be in [1, 14]";
    else if (p->mobility_weight < -127 || p->mobility_weight > 127) why = "mobility_weight must be in [-127, 127]";
    else if (p->terminal_weight < 1 || p->terminal_weight > 32767) why = "terminal_weight must be in [1, 32767]";
    else if (p->endgame_empties < 0 || p->endgame_empties > OTH_SEARCH_MAX_DEPTH)
        why = "endgame_empties must be in [0, 14]";
    else if (p->max_nodes < 1 || p->max_nodes > 0xffffffffull) why = "max_nodes must be in [1, 2^32 - 1]";
    if (!why) return OTH_OK;
    snprintf(msg, sizeof(msg), "search policy `%s`: %s", who, why);
    return fail(OTH_EINVAL, msg);
}
}  // namespace

extern "C" {

int oth_play_search(oth_env* env, const oth_search_policy* black, const oth_search_policy* white, int32_t n_plies,
                    int32_t* actions, int32_t* rewards, uint8_t* dones, uint8_t* fallbacks, oth_stream_t stream) {
    // the argument checks come before the handle is read
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (int rc = check_search_policy(black, "black")) return rc;
    if (int rc = check_search_policy(white, "white")) return rc;
    if (n_plies < 1) return fail(OTH_EINVAL, "n_plies must be >= 1");
    if (int rc = use_device(env)) return rc;
    const uint64_t ply0 = env->ply;
    env->ply += (uint64_t)n_plies;
    return with_n(env->n, [&](auto NC) {
        return launch_play_search<decltype(NC)::value>(env, OTH_PLAY_SEARCH_PLAY, black, white, n_plies, nullptr,
                                                       nullptr, nullptr, actions, rewards, dones, fallbacks, nullptr,
                                                       nullptr, ply0, (hipStream_t)stream);
    });
}

int oth_reset_vs_search(oth_env* env, const oth_search_policy* opponent, const int8_t* protagonist,
                        const uint8_t* mask, oth_stream_t stream) {
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (int rc = check_search_policy(opponent, "opponent")) return rc;
    if (int rc = use_device(env)) return rc;
    const uint64_t call = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_play_search<decltype(NC)::value>(env, OTH_PLAY_SEARCH_RESET_VS, opponent, opponent, 0, nullptr,
                                                       protagonist, mask, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                       nullptr, call, (hipStream_t)stream);
    });
}

int oth_step_vs_search(oth_env* env, const oth_search_policy* opponent, const int32_t* actions,
                       const int8_t* protagonist, int32_t* rewards, uint8_t* dones, int32_t* plies,
                       int32_t* fallbacks, oth_stream_t stream) {
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (int rc = check_search_policy(opponent, "opponent")) return rc;
    if (!actions) return fail(OTH_EINVAL, "actions is NULL");
    if (int rc = use_device(env)) return rc;
    const uint64_t call = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_play_search<decltype(NC)::value>(env, OTH_PLAY_SEARCH_STEP_VS, opponent, opponent, 0, actions,
                                                       protagonist, nullptr, nullptr, rewards, dones, nullptr, plies,
                                                       fallbacks, call, (hipStream_t)stream);
    });
}

}  // extern "C"

namespace {
// an oth_net_policy's ranges that need no handle; who: the argument's name for the message
int check_net_policy(const oth_net_policy* p, const char* who) {
    char msg[200];
    const char* why = nullptr;
    NetParams np;
    if (!p) why = "is NULL";
    else if (!p->blob) why = "has a NULL blob";
    else {
        np.layers = p->params.layers;
        np.width = p->params.width;
        for (int l = 0; l < 4; ++l) np.shift[l] = p->params.shift[l];
        np.policy_shift = p->params.policy_shift;
        np.value_shift = p->params.value_shift;
        why = net_check(8, &np);  // (the handle's board size is checked with blob_bytes, below)
        if (!why && (reinterpret_cast<uintptr_t>(p->blob) & 15u)) why = "blob must be 16-byte aligned";
        if (!why && (p->sample_discs < 0 || p->sample_discs > OTH_NET_SAMPLE_DISCS_MAX)) why = "sample_discs must be in [0, 257]";
    }
    if (!why) return OTH_OK;
    snprintf(msg, sizeof(msg), "net policy `%s`: %s", who, why);
    return fail(OTH_EINVAL, msg);
}
// ... and what needs the handle's board size
int check_net_policy_size(const oth_env* env, const oth_net_policy* p, const char* who) {
    char msg[200];
    NetParams np;
    np.layers = p->params.layers;
    np.width = p->params.width;
    for (int l = 0; l < 4; ++l) np.shift[l] = p->params.shift[l];
    np.policy_shift = p->params.policy_shift;
    np.value_shift = p->params.value_shift;
    const char* why = net_check(env->n, &np);
    if (!why && p->blob_bytes < net_geo(env->n, np).bytes()) why = "blob_bytes is below what oth_net_blob_bytes reports";
    if (!why) return OTH_OK;
    snprintf(msg, sizeof(msg), "net policy `%s`: %s", who, why);
    return fail(OTH_EINVAL, msg);
}
}  // namespace

extern "C" {

int oth_play_net(oth_env* env, const oth_net_policy* black, const oth_net_policy* white, int32_t n_plies,
                 int32_t* actions, int32_t* rewards, uint8_t* dones, oth_stream_t stream) {
    // the argument checks come before the handle is read
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (int rc = check_net_policy(black, "black")) return rc;
    if (int rc = check_net_policy(white, "white")) return rc;
    if (black->params.width != white->params.width)
        return fail(OTH_EINVAL, "the two networks of oth_play_net must have the same width");
    if (n_plies < 1) return fail(OTH_EINVAL, "n_plies must be >= 1");
    if (int rc = check_net_policy_size(env, black, "black")) return rc;
    if (int rc = check_net_policy_size(env, white, "white")) return rc;
    if (int rc = use_device(env)) return rc;
    const uint64_t ply0 = env->ply;
    env->ply += (uint64_t)n_plies;
    return with_n(env->n, [&](auto NC) {
        return launch_play_net<decltype(NC)::value>(env, OTH_PLAY_SEARCH_PLAY, black, white, n_plies, nullptr, nullptr,
                                                    nullptr, actions, rewards, dones, nullptr, ply0,
                                                    (hipStream_t)stream);
    });
}

int oth_reset_vs_net(oth_env* env, const oth_net_policy* opponent, const int8_t* protagonist, const uint8_t* mask,
                     oth_stream_t stream) {
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (int rc = check_net_policy(opponent, "opponent")) return rc;
    if (int rc = check_net_policy_size(env, opponent, "opponent")) return rc;
    if (int rc = use_device(env)) return rc;
    const uint64_t call = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_play_net<decltype(NC)::value>(env, OTH_PLAY_SEARCH_RESET_VS, opponent, opponent, 0, nullptr,
                                                    protagonist, mask, nullptr, nullptr, nullptr, nullptr, call,
                                                    (hipStream_t)stream);
    });
}

int oth_step_vs_net(oth_env* env, const oth_net_policy* opponent, const int32_t* actions, const int8_t* protagonist,
                    int32_t* rewards, uint8_t* dones, int32_t* plies, oth_stream_t stream) {
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (int rc = check_net_policy(opponent, "opponent")) return rc;
    if (!actions) return fail(OTH_EINVAL, "actions is NULL");
    if (int rc = check_net_policy_size(env, opponent, "opponent")) return rc;
    if (int rc = use_device(env)) return rc;
    const uint64_t call = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_play_net<decltype(NC)::value>(env, OTH_PLAY_SEARCH_STEP_VS, opponent, opponent, 0, actions,
                                                    protagonist, nullptr, nullptr, rewards, dones, plies, call,
                                                    (hipStream_t)stream);
    });
}

}  // extern "C"

namespace {
CnetParams cnet_params_of(const oth_cnet_params& q) {
    CnetParams cp;
    cp.channels = q.channels;
    cp.blocks = q.blocks;
    cp.shift_stem = q.shift_stem;
    for (int l = 0; l < 16; ++l) cp.shift[l] = q.shift[l];
    cp.shift_head = q.shift_head;
    cp.policy_shift = q.policy_shift;
    cp.value_shift = q.value_shift;
    return cp;
}
// an oth_cnet_policy's ranges that need no handle; who: the argument's name for the message
int check_cnet_policy(const oth_cnet_policy* p, const char* who) {
    char msg[200];
    const char* why = nullptr;
    if (!p) why = "is NULL";
    else if (!p->blob) why = "has a NULL blob";
    else {
        const CnetParams cp = cnet_params_of(p->params);
        why = cnet_check(8, &cp);  // (the handle's board size is checked with blob_bytes, below)
        if (!why && (reinterpret_cast<uintptr_t>(p->blob) & 15u)) why = "blob must be 16-byte aligned";
        if (!why && (p->sample_discs < 0 || p->sample_discs > OTH_NET_SAMPLE_DISCS_MAX)) why = "sample_discs must be in [0, 257]";
    }
    if (!why) return OTH_OK;
    snprintf(msg, sizeof(msg), "cnet policy `%s`: %s", who, why);
    return fail(OTH_EINVAL, msg);
}
// ... and what needs the handle's board size
int check_cnet_policy_size(const oth_env* env, const oth_cnet_policy* p, const char* who) {
    char msg[200];
    const CnetParams cp = cnet_params_of(p->params);
    const char* why = cnet_check(env->n, &cp);
    if (!why && p->blob_bytes < cnet_geo(env->n, cp).bytes()) why = "blob_bytes is below what oth_cnet_blob_bytes reports";
    if (!why) return OTH_OK;
    snprintf(msg, sizeof(msg), "cnet policy `%s`: %s", who, why);
    return fail(OTH_EINVAL, msg);
}
}  // namespace

extern "C" {

int oth_play_cnet(oth_env* env, const oth_cnet_policy* black, const oth_cnet_policy* white, int32_t n_plies,
                  int32_t* actions, int32_t* rewards, uint8_t* dones, oth_stream_t stream) {
    // the argument checks come before the handle is read
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (int rc = check_cnet_policy(black, "black")) return rc;
    if (int rc = check_cnet_policy(white, "white")) return rc;
    if (black->params.channels != white->params.channels)
        return fail(OTH_EINVAL, "the two networks of oth_play_cnet must have the same channels");
    if (n_plies < 1) return fail(OTH_EINVAL, "n_plies must be >= 1");
    if (int rc = check_cnet_policy_size(env, black, "black")) return rc;
    if (int rc = check_cnet_policy_size(env, white, "white")) return rc;
    if (int rc = use_device(env)) return rc;
    const uint64_t ply0 = env->ply;
    env->ply += (uint64_t)n_plies;
    return with_n(env->n, [&](auto NC) {
        return launch_play_cnet<decltype(NC)::value>(env, OTH_PLAY_SEARCH_PLAY, black, white, n_plies, nullptr, nullptr,
                                                     nullptr, actions, rewards, dones, nullptr, ply0,
                                                     (hipStream_t)stream);
    });
}

int oth_reset_vs_cnet(oth_env* env, const oth_cnet_policy* opponent, const int8_t* protagonist, const uint8_t* mask,
                      oth_stream_t stream) {
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (int rc = check_cnet_policy(opponent, "opponent")) return rc;
    if (int rc = check_cnet_policy_size(env, opponent, "opponent")) return rc;
    if (int rc = use_device(env)) return rc;
    const uint64_t call = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_play_cnet<decltype(NC)::value>(env, OTH_PLAY_SEARCH_RESET_VS, opponent, opponent, 0, nullptr,
                                                     protagonist, mask, nullptr, nullptr, nullptr, nullptr, call,
                                                     (hipStream_t)stream);
    });
}

int oth_step_vs_cnet(oth_env* env, const oth_cnet_policy* opponent, const int32_t* actions, const int8_t* protagonist,
                     int32_t* rewards, uint8_t* dones, int32_t* plies, oth_stream_t stream) {
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (int rc = check_cnet_policy(opponent, "opponent")) return rc;
    if (!actions) return fail(OTH_EINVAL, "actions is NULL");
    if (int rc = check_cnet_policy_size(env, opponent, "opponent")) return rc;
    if (int rc = use_device(env)) return rc;
    const uint64_t call = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_play_cnet<decltype(NC)::value>(env, OTH_PLAY_SEARCH_STEP_VS, opponent, opponent, 0, actions,
                                                     protagonist, nullptr, nullptr, rewards, dones, plies, call,
                                                     (hipStream_t)stream);
    });
}

}  // extern "C"

namespace {
// an oth_ntuple_policy against the handle's board size: the parameters, the device arguments, the search's ranges
// and the exploration's; who: the argument's name for the message; *key: what the plan's header must hold
int check_ntuple_policy(const oth_env* env, const oth_ntuple_policy* p, const char* who, NtupleKey* key) {
    char msg[200];
    if (!p) {
        snprintf(msg, sizeof(msg), "n-tuple policy `%s` is NULL", who);
        return fail(OTH_EINVAL, msg);
    }
    NtupleParams np;
    if (int rc = ntuple_params(env->n, &p->params, &np)) return rc;
    if (int rc = ntuple_device_args(np, p->plan, p->plan_bytes, p->weights, p->weight_count)) return rc;
    const char* why = nullptr;
    if (p->depth < 1 || p->depth > OTH_SEARCH_MAX_DEPTH) why = "depth must be in [1, 14]";
    else if (p->terminal_weight < 1 || p->terminal_weight > 32767) why = "terminal_weight must be in [1, 32767]";
    else if (p->endgame_empties < 0 || p->endgame_empties > OTH_SEARCH_MAX_DEPTH)
        why = "endgame_empties must be in [0, 14]";
    else if (p->explore < 0 || p->explore > OTH_NTUPLE_EXPLORE_ONE) why = "explore must be in [0, 65536]";
    else if (p->max_nodes < 1 || p->max_nodes > 0xffffffffull) why = "max_nodes must be in [1, 2^32 - 1]";
    if (why) {
        snprintf(msg, sizeof(msg), "n-tuple policy `%s`: %s", who, why);
        return fail(OTH_EINVAL, msg);
    }
    *key = ntuple_key(env->n, np);
    return OTH_OK;
}
}  // namespace

extern "C" {

int oth_play_ntuple(oth_env* env, const oth_ntuple_policy* black, const oth_ntuple_policy* white, int32_t n_plies,
                    int32_t* actions, int32_t* rewards, uint8_t* dones, uint8_t* fallbacks, const oth_ntuple_td* td,
                    oth_stream_t stream) {
    // the argument checks come before the handle's device is touched
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    NtupleKey kb, kw;
    if (int rc = check_ntuple_policy(env, black, "black", &kb)) return rc;
    if (int rc = check_ntuple_policy(env, white, "white", &kw)) return rc;
    if (n_plies < 1) return fail(OTH_EINVAL, "n_plies must be >= 1");
    if (td && (!td->boards || !td->meta || !td->targets || !td->learn))
        return fail(OTH_EINVAL, "a member of td is NULL");
    if (int rc = use_device(env)) return rc;
    const uint64_t ply0 = env->ply;
    env->ply += (uint64_t)n_plies;
    return with_n(env->n, [&](auto NC) {
        return launch_play_ntuple<decltype(NC)::value>(env, OTH_PLAY_SEARCH_PLAY, black, kb, white, kw, n_plies,
                                                       nullptr, nullptr, nullptr, actions, rewards, dones, fallbacks,
                                                       nullptr, nullptr, td, ply0, (hipStream_t)stream);
    });
}

int oth_reset_vs_ntuple(oth_env* env, const oth_ntuple_policy* opponent, const int8_t* protagonist,
                        const uint8_t* mask, oth_stream_t stream) {
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    NtupleKey key;
    if (int rc = check_ntuple_policy(env, opponent, "opponent", &key)) return rc;
    if (int rc = use_device(env)) return rc;
    const uint64_t call = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_play_ntuple<decltype(NC)::value>(env, OTH_PLAY_SEARCH_RESET_VS, opponent, key, opponent, key, 0,
                                                       nullptr, protagonist, mask, nullptr, nullptr, nullptr, nullptr,
                                                       nullptr, nullptr, nullptr, call, (hipStream_t)stream);
    });
}

int oth_step_vs_ntuple(oth_env* env, const oth_ntuple_policy* opponent, const int32_t* actions,
                       const int8_t* protagonist, int32_t* rewards, uint8_t* dones, int32_t* plies,
                       int32_t* fallbacks, oth_stream_t stream) {
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    NtupleKey key;
    if (int rc = check_ntuple_policy(env, opponent, "opponent", &key)) return rc;
    if (!actions) return fail(OTH_EINVAL, "actions is NULL");
    if (int rc = use_device(env)) return rc;
    const uint64_t call = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_play_ntuple<decltype(NC)::value>(env, OTH_PLAY_SEARCH_STEP_VS, opponent, key, opponent, key, 0,
                                                       actions, protagonist, nullptr, nullptr, rewards, dones, nullptr,
                                                       plies, fallbacks, nullptr, call, (hipStream_t)stream);
    });
}

int oth_reset_vs(oth_env* env, int32_t opponent_policy, const int8_t* protagonist, const uint8_t* mask,
                 oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (opponent_policy < OTH_POLICY_RANDOM || opponent_policy > OTH_POLICY_LAST)
        return fail(OTH_EINVAL, "unknown opponent policy");
    if (int rc = maximin_budget(env, opponent_policy, 2.0, MM_RESET_VS, (hipStream_t)stream)) return rc;
    const uint64_t call = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_reset_vs<decltype(NC)::value>(env, opponent_policy, protagonist, mask, call,
                                                    (hipStream_t)stream);
    });
}

int oth_step_vs(oth_env* env, int32_t opponent_policy, const int32_t* actions, const int8_t* protagonist,
                int32_t* rewards, uint8_t* dones, int32_t* plies, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (!actions) return fail(OTH_EINVAL, "actions is NULL");
    if (opponent_policy < OTH_POLICY_RANDOM || opponent_policy > OTH_POLICY_LAST)
        return fail(OTH_EINVAL, "unknown opponent policy");
    if (int rc = maximin_budget(env, opponent_policy, 2.0, MM_STEP_VS, (hipStream_t)stream)) return rc;
    const uint64_t call = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_step_vs<decltype(NC)::value>(env, opponent_policy, actions, protagonist, rewards, dones,
                                                   plies, call, -1, 0, nullptr, (hipStream_t)stream);
    });
}

int oth_step_vs_observe(oth_env* env, int32_t opponent_policy, const int32_t* actions, const int8_t* protagonist,
                        int32_t* rewards, uint8_t* dones, int32_t* plies, int32_t layout, int32_t dtype, void* obs,
                        oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (!actions || !obs) return fail(OTH_EINVAL, "actions / obs is NULL");
    if (opponent_policy < OTH_POLICY_RANDOM || opponent_policy > OTH_POLICY_LAST)
        return fail(OTH_EINVAL, "unknown opponent policy");
    if (layout < OTH_OBS_BOARD || layout > OTH_OBS_LEGAL) return fail(OTH_EINVAL, "unknown layout");
    if (dtype < OTH_I8 || dtype > OTH_BF16) return fail(OTH_EINVAL, "unknown dtype");
    if (int rc = maximin_budget(env, opponent_policy, 2.0, MM_STEP_VS, (hipStream_t)stream)) return rc;
    const uint64_t call = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_step_vs<decltype(NC)::value>(env, opponent_policy, actions, protagonist, rewards, dones,
                                                   plies, call, layout, dtype, obs, (hipStream_t)stream);
    });
}

int oth_policy_actions(oth_env* env, int32_t policy, int32_t* out, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (!out) return fail(OTH_EINVAL, "out is NULL");
    if (policy < OTH_POLICY_GREEDY || policy > OTH_POLICY_LAST)
        return fail(OTH_EINVAL, "policy must be greedy or maximin (depth 1 .. OTH_MAXIMIN_MAX_DEPTH)");
    if (int rc = maximin_budget(env, policy, 1.0, MM_POLICY, (hipStream_t)stream)) return rc;
    return with_n(env->n, [&](auto NC) {
        return launch_policy_actions<decltype(NC)::value>(env, policy, out, (hipStream_t)stream);
    });
}

int oth_greedy_actions(oth_env* env, int32_t* out, oth_stream_t stream) {
    return oth_policy_actions(env, OTH_POLICY_GREEDY, out, stream);
}

int oth_legal(oth_env* env, uint64_t* out, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (!out) return fail(OTH_EINVAL, "out is NULL");
    OTH_HIP(hipMemcpyAsync(out, env->legal, (size_t)env->E * env->W * sizeof(uint64_t), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    return OTH_OK;
}

int oth_legal_moves(int32_t board_size, int32_t n, const uint64_t* mover, const uint64_t* opp, uint64_t* out,
                    oth_stream_t stream) {
    if (n < 0 || (n > 0 && (!mover || !opp || !out))) return fail(OTH_EINVAL, "bad arguments");
    if (n == 0) return OTH_OK;
    const int bs = board_size < 4 ? 4 : board_size;
    return with_n(bs, [&](auto NC) {
        return launch_legal_moves<decltype(NC)::value>(n, mover, opp, out, (hipStream_t)stream);
    });
}


int oth_masked_sample(int32_t board_size, int32_t n, const float* logits, int64_t ld, const uint64_t* legal,
                      const float* uniforms, uint64_t seed, uint32_t id_base, uint64_t counter, int32_t mode,
                      int32_t* actions, float* log_probs, float* entropy, oth_stream_t stream) {
    const int bs = board_size < 4 ? 4 : board_size;
    if (bs > 16) return fail(OTH_EINVAL, "board_size must be <= 16");
    if ((mode & ~OTH_MASKED_FULL_ENTROPY) < OTH_MASKED_SAMPLE || (mode & ~OTH_MASKED_FULL_ENTROPY) > OTH_MASKED_EVAL)
        return fail(OTH_EINVAL, "unknown mode");
    if (n < 0 || (n > 0 && (!logits || !legal || !actions))) return fail(OTH_EINVAL, "bad arguments");
    if (ld < (int64_t)bs * bs) return fail(OTH_EINVAL, "ld < board_size^2");
    if (n == 0) return OTH_OK;
    return launch_masked(bs, n, logits, (long long)ld, legal, uniforms, seed, id_base, counter, nullptr, mode, actions,
                         log_probs, entropy, (hipStream_t)stream);
}

int oth_sample_actions(oth_env* env, const float* logits, int64_t ld, const float* uniforms, uint64_t counter,
                       int32_t mode, int32_t* actions, float* log_probs, float* entropy, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (!logits || !actions) return fail(OTH_EINVAL, "logits / actions is NULL");
    if ((mode & ~OTH_MASKED_FULL_ENTROPY) < OTH_MASKED_SAMPLE || (mode & ~OTH_MASKED_FULL_ENTROPY) > OTH_MASKED_EVAL)
        return fail(OTH_EINVAL, "unknown mode");
    if (ld < (int64_t)env->n * env->n) return fail(OTH_EINVAL, "ld < N*N");
    return launch_masked(env->n, env->E, logits, (long long)ld, env->legal, uniforms, env->seed, env->id_base, counter,
                         env->cur_off + 1, mode, actions, log_probs, entropy, (hipStream_t)stream);
}

int oth_sample_step(oth_env* env, const float* logits, int64_t ld, const float* uniforms, uint64_t counter,
                    int32_t mode, int32_t* actions, float* log_probs, float* entropy, int32_t* rewards, uint8_t* dones,
                    oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (!logits || !actions) return fail(OTH_EINVAL, "logits / actions is NULL");
    const int base = mode & ~OTH_MASKED_FULL_ENTROPY;
    if (base != OTH_MASKED_SAMPLE && base != OTH_MASKED_MODE) return fail(OTH_EINVAL, "mode must be SAMPLE or MODE");
    if (ld < (int64_t)env->n * env->n) return fail(OTH_EINVAL, "ld < N*N");
    const uint64_t ply = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_sample_step<decltype(NC)::value>(env, logits, (long long)ld, uniforms, counter, mode, actions,
                                                       log_probs, entropy, rewards, dones, ply, -1, 0, nullptr,
                                                       (hipStream_t)stream);
    });
}

int oth_sample_step_observe(oth_env* env, const float* logits, int64_t ld, const float* uniforms, uint64_t counter,
                            int32_t mode, int32_t* actions, float* log_probs, float* entropy, int32_t* rewards,
                            uint8_t* dones, int32_t layout, int32_t dtype, void* obs, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (!logits || !actions || !obs) return fail(OTH_EINVAL, "logits / actions / obs is NULL");
    const int base = mode & ~OTH_MASKED_FULL_ENTROPY;
    if (base != OTH_MASKED_SAMPLE && base != OTH_MASKED_MODE) return fail(OTH_EINVAL, "mode must be SAMPLE or MODE");
    if (ld < (int64_t)env->n * env->n) return fail(OTH_EINVAL, "ld < N*N");
    if (layout < OTH_OBS_BOARD || layout > OTH_OBS_LEGAL) return fail(OTH_EINVAL, "unknown layout");
    if (dtype < OTH_I8 || dtype > OTH_BF16) return fail(OTH_EINVAL, "unknown dtype");
    const uint64_t ply = env->ply++;
    return with_n(env->n, [&](auto NC) {
        return launch_sample_step<decltype(NC)::value>(env, logits, (long long)ld, uniforms, counter, mode, actions,
                                                       log_probs, entropy, rewards, dones, ply, layout, dtype, obs,
                                                       (hipStream_t)stream);
    });
}

// A graph region's offsets move on by what one replay consumed (enqueued as
// the region's last node, so every replay advances them).
__global__ void k_graph_advance(uint64_t* __restrict__ off, uint64_t d_ply, uint64_t d_sample) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        off[0] += d_ply;
        off[1] += d_sample;
    }
}

int oth_graph_begin(oth_env* env, int32_t* slot) {
    if (!env || !slot) return fail(OTH_EINVAL, "NULL argument");
    if (env->graph_slot) return fail(OTH_EINVAL, "a graph region is already open on this handle");
    if (env->slots_used == ~0ull)
        return fail(OTH_EINVAL, "no graph counter slot left on this handle (oth_graph_release frees one)");
    const int k = __builtin_ctzll(~env->slots_used);  // the lowest free slot
    env->slots_used |= 1ull << k;
    env->graph_slot = k;
    env->ply_saved = env->ply;
    env->ply = (uint64_t)k << OTH_GRAPH_COUNTER_SHIFT;
    env->cur_off = env->ctr_slots + 2 * k;
    *slot = k;
    return OTH_OK;
}

int oth_graph_end(oth_env* env, uint64_t d_sample, int32_t enqueue, uint64_t* d_ply, oth_stream_t stream) {
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (!env->graph_slot) return fail(OTH_EINVAL, "no graph region is open on this handle");
    const int k = env->graph_slot;
    const uint64_t dp = env->ply - ((uint64_t)k << OTH_GRAPH_COUNTER_SHIFT);
    env->ply = env->ply_saved;  // eager counting resumes where it was
    env->cur_off = env->ctr_slots;
    env->graph_slot = 0;
    if (d_ply) *d_ply = dp;
    if (!enqueue) return OTH_OK;
    OTH_CHECK_ENV(env);
    launch_k(k_graph_advance, dim3(1), dim3(64), 0, (hipStream_t)stream, env->ctr_slots + 2 * k, dp,
             d_sample);
    return oth_host::after_launch("oth_graph_end");
}

// A released slot keeps its device offsets: a later region on it draws past
// every counter the earlier graph drew, so ranges stay disjoint even if that
// graph is still replayed.
int oth_graph_release(oth_env* env, int32_t slot) {
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (slot <= 0 || slot >= OTH_GRAPH_SLOTS) return fail(OTH_EINVAL, "slot out of range");
    if (slot == env->graph_slot) return fail(OTH_EINVAL, "the slot's graph region is still open");
    env->slots_used &= ~(1ull << slot);
    return OTH_OK;
}

int oth_graph_offsets(const oth_env* env, int32_t slot, uint64_t* out) {
    OTH_CHECK_ENV(env);
    if (!out) return fail(OTH_EINVAL, "out is NULL");
    if (slot < 0 || slot >= OTH_GRAPH_SLOTS) return fail(OTH_EINVAL, "slot out of range");
    OTH_HIP(hipDeviceSynchronize());
    OTH_HIP(hipMemcpy(out, env->ctr_slots + 2 * slot, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return OTH_OK;
}

int oth_observe(oth_env* env, int32_t layout, int32_t dtype, void* out, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (!out) return fail(OTH_EINVAL, "out is NULL");
    if (layout < OTH_OBS_BOARD || layout > OTH_OBS_LEGAL) return fail(OTH_EINVAL, "unknown layout");
    if (dtype < OTH_I8 || dtype > OTH_BF16) return fail(OTH_EINVAL, "unknown dtype");
    return with_n(env->n, [&](auto NC) {
        return launch_observe<decltype(NC)::value>(env, layout, dtype, out, (hipStream_t)stream);
    });
}

int oth_get_state(oth_env* env, uint64_t* boards, uint16_t* meta, uint64_t* legal, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    const size_t E = (size_t)env->E, W = (size_t)env->W;
    hipStream_t s = (hipStream_t)stream;
    if (boards) OTH_HIP(hipMemcpyAsync(boards, env->boards, E * 2 * W * 8, hipMemcpyDefault, s));
    if (meta) OTH_HIP(hipMemcpyAsync(meta, env->meta, E * 2, hipMemcpyDefault, s));
    if (legal) OTH_HIP(hipMemcpyAsync(legal, env->legal, E * W * 8, hipMemcpyDefault, s));
    return OTH_OK;
}

int oth_set_state(oth_env* env, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal,
                  oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    const size_t E = (size_t)env->E, W = (size_t)env->W;
    hipStream_t s = (hipStream_t)stream;
    if (boards) OTH_HIP(hipMemcpyAsync(env->boards, boards, E * 2 * W * 8, hipMemcpyDefault, s));
    if (meta) OTH_HIP(hipMemcpyAsync(env->meta, meta, E * 2, hipMemcpyDefault, s));
    if (legal) OTH_HIP(hipMemcpyAsync(env->legal, legal, E * W * 8, hipMemcpyDefault, s));
    return OTH_OK;
}

int oth_set_player_turn(oth_env* env, int32_t turn, const uint8_t* mask, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (turn != 1 && turn != -1) return fail(OTH_EINVAL, "turn must be +1 or -1");
    return with_n(env->n, [&](auto NC) {
        return launch_set_turn<decltype(NC)::value>(env, turn, mask, (hipStream_t)stream);
    });
}

int oth_count_disks(oth_env* env, int32_t* out, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (!out) return fail(OTH_EINVAL, "out is NULL");
    return with_n(env->n, [&](auto NC) { return launch_count<decltype(NC)::value>(env, out, (hipStream_t)stream); });
}

int oth_counts(oth_env* env, int64_t* out, int32_t reset, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (!out) return fail(OTH_EINVAL, "out is NULL");
    hipStream_t s = (hipStream_t)stream;
    launch_k(k_reduce_wdl, dim3(1), dim3(256), 0, s, env->wdl, env->nslots, out, reset ? 1 : 0);
    return after_launch("oth_counts");
}

int oth_counts_vs(oth_env* env, int64_t* out, int32_t reset, oth_stream_t stream) {
    OTH_CHECK_ENV(env);
    if (!out) return fail(OTH_EINVAL, "out is NULL");
    launch_k(k_reduce_wdl, dim3(1), dim3(256), 0, (hipStream_t)stream, env->wdl_vs, env->nslots, out,
             reset ? 1 : 0);
    return after_launch("oth_counts_vs");
}

uint64_t oth_ply_counter(const oth_env* env) { return env ? env->ply : 0; }

int oth_set_ply_counter(oth_env* env, uint64_t ply) {
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (env->graph_slot) return fail(OTH_EINVAL, "cannot set the ply counter inside a graph region");
    env->ply = ply;  // host only: graph regions keep their own counter ranges
    return OTH_OK;
}

int oth_shape(const oth_env* env, int32_t* n_envs, int32_t* board_size, int32_t* words) {
    if (!env) return fail(OTH_EINVAL, "NULL oth_env");
    if (n_envs) *n_envs = env->E;
    if (board_size) *board_size = env->n;
    if (words) *words = env->W;
    return OTH_OK;
}

}  // extern "C"
