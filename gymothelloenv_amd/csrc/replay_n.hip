// replay_n.hip -- k_replay_begin, k_replay_append, k_replay_label, k_replay_count, k_replay_scan and
// k_replay_batch (oth_replay_begin / _append / _label / _counts / _gather / _sample: the self-play
// samples kept, labelled and drawn on the device, replay.hpp) and k_symmetry_masks (oth_symmetry_masks)
// in a translation unit of its own per board size (-DOTH_N=4 .. 16), like puct_n.hip.
#include "replay.hpp"
#include "launch.hpp"

#ifndef OTH_N
#error "compile with -DOTH_N=<board size>"
#endif

using namespace oth;
using namespace oth_dev;

namespace oth_host {

static_assert(replay_ws_words(OTH_N, 1, 1, 1) == replay_workspace_words(OTH_N, 1, 1, 1) &&
                  replay_ws_words(OTH_N, 37, 31, 4096) == replay_workspace_words(OTH_N, 37, 31, 4096) &&
                  replay_ws_words(OTH_N, 256, 65536, 1 << 20) == replay_workspace_words(OTH_N, 256, 65536, 1 << 20),
              "oth_replay_workspace_bytes' layout");

namespace {

unsigned replay_grid(long long n, int block) { return (unsigned)((n + block - 1) / block); }

template <int N>
ReplayWs<N> replay_ws(const oth_env* env, int H, int B, void* workspace) {
    return ReplayWs<N>{reinterpret_cast<uint64_t*>(workspace), (uint32_t)env->E, (uint32_t)H, (uint32_t)B};
}

// the rank step's two launches: the chunks' counts, then their prefix (and oth_replay_counts' out)
template <int N>
void replay_rank(const ReplayWs<N>& ws, int64_t* counts, hipStream_t st) {
    launch_k(k_replay_count<N>, dim3((unsigned)ws.chunks()), dim3(REPLAY_COUNT_BLOCK), 0, st, (int)ws.E, ws.H, ws.B,
             ws.base);
    launch_k(k_replay_scan<N>, dim3(1), dim3(REPLAY_SCAN_BLOCK), 0, st, (int)ws.E, ws.H, ws.B, ws.base, counts);
}

}  // namespace

template <int N>
int launch_replay_begin(oth_env* env, int H, int B, void* workspace, hipStream_t st) {
    const ReplayWs<N> ws = replay_ws<N>(env, H, B, workspace);
    const long long words = (long long)((ws.rows() + 7) / 8);
    launch_k(k_replay_begin<N>, dim3(replay_grid(words > env->E ? words : env->E, 256)), dim3(256), 0, st, env->E,
             ws.H, ws.B, ws.base);
    return after_launch("oth_replay_begin");
}

template <int N>
int launch_replay_append(oth_env* env, int H, int B, void* workspace, const int32_t* visits, const uint8_t* skip,
                         hipStream_t st) {
    const ReplayWs<N> ws = replay_ws<N>(env, H, B, workspace);
    launch_k(k_replay_append<N>, dim3(replay_grid(env->E, REPLAY_BLOCK)), dim3(REPLAY_BLOCK), 0, st, env->boards,
             env->meta, env->legal, env->E, ws.H, ws.B, ws.base, visits, skip);
    return after_launch("oth_replay_append");
}

template <int N>
int launch_replay_label(oth_env* env, int H, int B, void* workspace, const int32_t* rewards, const uint8_t* dones,
                        hipStream_t st) {
    const ReplayWs<N> ws = replay_ws<N>(env, H, B, workspace);
    launch_k(k_replay_label<N>, dim3(replay_grid(env->E, REPLAY_BLOCK)), dim3(REPLAY_BLOCK), 0, st, env->E, ws.H,
             ws.B, ws.base, rewards, dones);
    return after_launch("oth_replay_label");
}

template <int N>
int launch_replay_counts(oth_env* env, int H, int B, void* workspace, int64_t* out, hipStream_t st) {
    replay_rank<N>(replay_ws<N>(env, H, B, workspace), out, st);
    return after_launch("oth_replay_counts");
}

template <int N>
int launch_replay_batch(oth_env* env, int H, int B, void* workspace, int n, const int32_t* rows_in,
                        const uint8_t* sym_in, int augment, uint64_t seed, uint32_t id_key, uint64_t counter,
                        const oth_replay_batch* b, hipStream_t st) {
    const ReplayWs<N> ws = replay_ws<N>(env, H, B, workspace);
    const char* what = rows_in ? "oth_replay_gather" : "oth_replay_sample";
    if (!rows_in) replay_rank<N>(ws, nullptr, st);
    // the exchange format of the batch: the caller's arrays where given, else the staging rows
    uint64_t* boards = b->boards ? b->boards : ws.stage_boards();
    uint16_t* meta = b->meta ? b->meta : ws.stage_meta();
    uint64_t* legal = b->legal ? b->legal : ws.stage_legal();
    launch_k(k_replay_batch<N>, dim3(replay_grid(n, REPLAY_BLOCK)), dim3(REPLAY_BLOCK), 0, st, env->E, ws.H, ws.B,
             ws.base, n, rows_in, sym_in, augment, seed, id_key, counter,
             ReplayBatch{b->state, b->boards, b->meta, b->legal, b->visits, b->outcome, b->rows, b->sym}, boards, meta,
             legal);
    if (int rc = after_launch(what)) return rc;
    if (!b->obs) return OTH_OK;
    oth_env view = *env;  // launch_observe reads the geometry and these three pointers
    view.E = n;
    view.boards = boards;
    view.meta = meta;
    view.legal = legal;
    return launch_observe<N>(&view, b->layout, b->dtype, b->obs, st);
}

template <int N>
int launch_symmetry_masks(int n, int planes, const uint8_t* sym, const uint64_t* in, uint64_t* out, hipStream_t st) {
    const long long total = (long long)n * planes;
    launch_k(k_symmetry_masks<N>, dim3(replay_grid(total, 256)), dim3(256), 0, st, total, planes, sym, in, out);
    return after_launch("oth_symmetry_masks");
}

template int launch_replay_begin<OTH_N>(oth_env*, int, int, void*, hipStream_t);
template int launch_replay_append<OTH_N>(oth_env*, int, int, void*, const int32_t*, const uint8_t*, hipStream_t);
template int launch_replay_label<OTH_N>(oth_env*, int, int, void*, const int32_t*, const uint8_t*, hipStream_t);
template int launch_replay_counts<OTH_N>(oth_env*, int, int, void*, int64_t*, hipStream_t);
template int launch_replay_batch<OTH_N>(oth_env*, int, int, void*, int, const int32_t*, const uint8_t*, int, uint64_t,
                                        uint32_t, uint64_t, const oth_replay_batch*, hipStream_t);
template int launch_symmetry_masks<OTH_N>(int, int, const uint8_t*, const uint64_t*, uint64_t*, hipStream_t);

}  // namespace oth_host
