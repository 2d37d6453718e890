// ntuple_n.hip -- k_ntuple_eval (oth_ntuple_eval), k_ntuple_delta and k_ntuple_add (oth_ntuple_update's and
// oth_ntuple_update_masked's two launches) and k_search_ntuple (oth_search_ntuple): the n-tuple network of ntuple.hpp in a translation unit of
// its own per board size (-DOTH_N=4 .. 16), like search_n.hip.
//
// Rows (eval, delta, add): a group of NTUPLE_LANES = 8 lanes a row, lane s of the group taking symmetry s.  The
// block copies the plan (at most 2,336 bytes) into LDS once; a lane reads its row's words (the group's eight loads
// of one address are one request), walks the T tuples of its symmetry -- T independent gathers from the weights,
// which stay in global memory (at most 840 KB: L2-resident) -- and the group adds its eight int64 shares by three
// xor shuffles.  Lane 0 of the group adds the bias and stores.  The add kernel maps the same way: a lane adds the
// row's delta to the T entries of its symmetry with device-scope relaxed atomics on uint32, lane 0 to the bias as
// well.  Integer addition commutes, so neither the mapping nor the order of arrival shows in the weights.
//
// The search: root_tasks.hpp's kernel body, a lane a root move, with the plan in LDS where oth_search keeps its
// bit-planes; a lane at a frontier leaf walks all 8 T entries itself.
#include "ntuple.hpp"
#include "launch.hpp"

#ifndef OTH_N
#error "compile with -DOTH_N=<board size>"
#endif

using namespace oth;
using namespace oth_dev;

static_assert(NTUPLE_MAX_TUPLES == OTH_NTUPLE_MAX_TUPLES && NTUPLE_MAX_LENGTH == OTH_NTUPLE_MAX_LENGTH &&
                  NTUPLE_MAX_ROWS == OTH_NTUPLE_MAX_ROWS && NTUPLE_VALUE_ONE == OTH_PUCT_VALUE_ONE,
              "the header's limits");

namespace oth_dev {

constexpr int NTUPLE_BLOCK = 256, NTUPLE_LANES = 8, NTUPLE_ROWS = NTUPLE_BLOCK / NTUPLE_LANES;
constexpr int NTUPLE_PLAN_WORDS = NTUPLE_HEAD + NTUPLE_REC * NTUPLE_MAX_TUPLES;

// The plan into LDS (key.tuples is checked: at most 32) and whether it is the one the call names:
// block-uniform.  To be called by every lane of the block.
__device__ __forceinline__ bool plan_to_lds(const uint32_t* __restrict__ plan, const NtupleKey& key, uint32_t* lds) {
    const int words = NTUPLE_HEAD + NTUPLE_REC * (int)key.tuples;
    for (int i = threadIdx.x; i < words; i += blockDim.x) lds[i] = plan[i];
    __syncthreads();
    return ntuple_plan_is(lds, key);
}

// The row of the lane's group (r < R), its symmetry's share summed over the group: S on every lane of it
template <int W>
__device__ __forceinline__ int64_t group_sum(const uint32_t* lds, const NtupleKey& key, const int32_t* __restrict__ w,
                                             const uint64_t* __restrict__ boards, const uint16_t* __restrict__ meta,
                                             size_t r, int s) {
    uint64_t M[W], O[W];
    ntuple_row<W>(boards, meta, r, M, O);
    long long acc = ntuple_sum_sym(lds, (int)key.tuples, s, w, M, O);
#pragma unroll
    for (int m = 1; m < NTUPLE_LANES; m <<= 1) acc += __shfl_xor(acc, m);
    return (int64_t)acc + (int64_t)w[key.n_weights];
}

template <int N>
__global__ __launch_bounds__(NTUPLE_BLOCK) void k_ntuple_eval(int R, const uint32_t* __restrict__ plan, NtupleKey key,
                                                              const int32_t* __restrict__ w,
                                                              const uint64_t* __restrict__ boards,
                                                              const uint16_t* __restrict__ meta,
                                                              int32_t* __restrict__ values, int64_t* __restrict__ sums) {
    __shared__ uint32_t g_plan[NTUPLE_PLAN_WORDS];
    if (!plan_to_lds(plan, key, g_plan)) return;
    const long long r = (long long)blockIdx.x * NTUPLE_ROWS + threadIdx.x / NTUPLE_LANES;
    const int s = threadIdx.x % NTUPLE_LANES;
    // (a group past R works on the last row and stores nothing: every lane of a wave takes the shuffles)
    const int64_t S = group_sum<Geo<N>::W>(g_plan, key, w, boards, meta, (size_t)(r < R ? r : R - 1), s);
    if (r < R && s == 0) {
        values[r] = ntuple_value(S, (int)key.shift);
        if (sums) sums[r] = S;
    }
}

template <int N>
__global__ __launch_bounds__(NTUPLE_BLOCK) void k_ntuple_delta(int R, const uint32_t* __restrict__ plan, NtupleKey key,
                                                               const int32_t* __restrict__ w,
                                                               const uint64_t* __restrict__ boards,
                                                               const uint16_t* __restrict__ meta,
                                                               const int32_t* __restrict__ targets,
                                                               const uint8_t* __restrict__ mask, int32_t rate,
                                                               int rate_shift, int32_t* __restrict__ deltas) {
    __shared__ uint32_t g_plan[NTUPLE_PLAN_WORDS];
    if (!plan_to_lds(plan, key, g_plan)) return;
    const long long r = (long long)blockIdx.x * NTUPLE_ROWS + threadIdx.x / NTUPLE_LANES;
    const int s = threadIdx.x % NTUPLE_LANES;
    const int64_t S = group_sum<Geo<N>::W>(g_plan, key, w, boards, meta, (size_t)(r < R ? r : R - 1), s);
    // (a row the mask leaves out: d = 0, which k_ntuple_add skips)
    if (r < R && s == 0)
        deltas[r] = mask && !mask[r] ? 0 : ntuple_delta(targets[r], ntuple_value(S, (int)key.shift), rate, rate_shift);
}

template <int N>
__global__ __launch_bounds__(NTUPLE_BLOCK) void k_ntuple_add(int R, const uint32_t* __restrict__ plan, NtupleKey key,
                                                             uint32_t* w, const uint64_t* __restrict__ boards,
                                                             const uint16_t* __restrict__ meta,
                                                             const int32_t* __restrict__ deltas) {
    constexpr int W = Geo<N>::W;
    __shared__ uint32_t g_plan[NTUPLE_PLAN_WORDS];
    if (!plan_to_lds(plan, key, g_plan)) return;
    const long long r = (long long)blockIdx.x * NTUPLE_ROWS + threadIdx.x / NTUPLE_LANES;
    const int s = threadIdx.x % NTUPLE_LANES;
    if (r >= R) return;
    const uint32_t d = (uint32_t)deltas[r];
    if (d == 0u) return;  // (adds nothing)
    uint64_t M[W], O[W];
    ntuple_row<W>(boards, meta, (size_t)r, M, O);
    for (int t = 0; t < (int)key.tuples; ++t) {
        const uint32_t e = ntuple_entry(g_plan + NTUPLE_HEAD + NTUPLE_REC * t, s, M, O);
        if (e < key.n_weights) atomicAdd(&w[e], d);  // (always, for a plan of these parameters)
    }
    if (s == 0) atomicAdd(&w[key.n_weights], d);
}

template <int N>
__global__ __launch_bounds__(SOLVE_BLOCK) void k_search_ntuple(const uint64_t* __restrict__ boards,
                                                               const uint16_t* __restrict__ meta,
                                                               const uint64_t* __restrict__ legal, int E, int depth,
                                                               const uint32_t* __restrict__ plan, NtupleKey key,
                                                               const int32_t* __restrict__ weights, int terminal,
                                                               uint32_t max_nodes, int32_t* __restrict__ value,
                                                               int32_t* __restrict__ best,
                                                               int32_t* __restrict__ move_values,
                                                               uint8_t* __restrict__ status,
                                                               unsigned long long* __restrict__ nodes) {
    using Board = BB<Geo<N>::W>;
    __shared__ uint32_t g_plan[NTUPLE_PLAN_WORDS];
    if (!plan_to_lds(plan, key, g_plan)) return;
    const NtupleEval ev{g_plan, weights, terminal};
    root_tasks_kernel<N, SearchFrame<N>>(
        boards, meta, legal, E, value, best, move_values, status, nodes,
        [&](const Board& B, const Board& Wt, const Board& Lg, uint32_t m, int& v) {
            return search_status<N>(B, Wt, Lg, m, terminal, v);
        },
        [&](RootTask<N>& s, uint32_t* st) { ntuple_search_step<N>(s, st, max_nodes, depth, ev); });
}

}  // namespace oth_dev

namespace oth_host {

// (of checked arguments; n_rows >= 1)
template <int N>
int launch_ntuple_eval(int n_rows, const void* plan, const NtupleKey& key, const int32_t* weights, const uint64_t* boards,
                       const uint16_t* meta, int32_t* values, int64_t* sums, hipStream_t st) {
    const dim3 grid((unsigned)(((long long)n_rows + NTUPLE_ROWS - 1) / NTUPLE_ROWS)), block(NTUPLE_BLOCK);
    launch_k(k_ntuple_eval<N>, grid, block, 0, st, n_rows, static_cast<const uint32_t*>(plan), key, weights, boards, meta,
             values, sums);
    return after_launch("oth_ntuple_eval");
}

template <int N>
int launch_ntuple_update(int n_rows, const void* plan, const NtupleKey& key, int32_t* weights, const uint64_t* boards,
                         const uint16_t* meta, const int32_t* targets, const uint8_t* mask, int32_t rate, int rate_shift,
                         int32_t* deltas, hipStream_t st) {
    const dim3 grid((unsigned)(((long long)n_rows + NTUPLE_ROWS - 1) / NTUPLE_ROWS)), block(NTUPLE_BLOCK);
    launch_k(k_ntuple_delta<N>, grid, block, 0, st, n_rows, static_cast<const uint32_t*>(plan), key,
             static_cast<const int32_t*>(weights), boards, meta, targets, mask, rate, rate_shift, deltas);
    launch_k(k_ntuple_add<N>, grid, block, 0, st, n_rows, static_cast<const uint32_t*>(plan), key,
             reinterpret_cast<uint32_t*>(weights), boards, meta, static_cast<const int32_t*>(deltas));
    return after_launch("oth_ntuple_update");
}

template <int N>
int launch_search_ntuple(oth_env* env, int depth, const void* plan, const NtupleKey& key, const int32_t* weights,
                         int terminal, uint32_t max_nodes, int32_t* value, int32_t* best, int32_t* move_values,
                         uint8_t* status, uint64_t* nodes, hipStream_t st) {
    const long long groups = ((long long)env->E + SOLVE_GROUP - 1) / SOLVE_GROUP;
    launch_k(k_search_ntuple<N>, dim3((unsigned)groups), dim3(SOLVE_BLOCK), 0, st, env->boards, env->meta, env->legal,
             env->E, depth, static_cast<const uint32_t*>(plan), key, weights, terminal, max_nodes, value, best,
             move_values, status, reinterpret_cast<unsigned long long*>(nodes));
    return after_launch("oth_search_ntuple");
}

template int launch_ntuple_eval<OTH_N>(int, const void*, const NtupleKey&, const int32_t*, const uint64_t*,
                                       const uint16_t*, int32_t*, int64_t*, hipStream_t);
template int launch_ntuple_update<OTH_N>(int, const void*, const NtupleKey&, int32_t*, const uint64_t*, const uint16_t*,
                                         const int32_t*, const uint8_t*, int32_t, int, int32_t*, hipStream_t);
template int launch_search_ntuple<OTH_N>(oth_env*, int, const void*, const NtupleKey&, const int32_t*, int, uint32_t,
                                         int32_t*, int32_t*, int32_t*, uint8_t*, uint64_t*, hipStream_t);

}  // namespace oth_host
