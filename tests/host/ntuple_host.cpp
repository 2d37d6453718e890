// Host build of the n-tuple network (csrc/ntuple.hpp: the parameter check, the plan, the cell code,
// index, sum, value and delta of a row, the additions and the search's node step -- the text the
// device kernels run, compiled with g++) for tests/test_ntuple_host.py: a shared library with C
// linkage that has the oth_ntuple_* calls on host memory.  tests/host/ntuple_san_main.cpp includes
// this file under -fsanitize=address,undefined.  Test infrastructure only.
#include <stdint.h>
#include <string.h>

#include "../../gymothelloenv_amd/csrc/ntuple.hpp"

using namespace oth;

namespace {

constexpr int PLAN_WORDS = NTUPLE_HEAD + NTUPLE_REC * NTUPLE_MAX_TUPLES;

// the checked parameters and their plan; false: out of range
bool make_plan(int n, const NtupleParams* p, uint32_t* plan) {
    if (!p || ntuple_check(n, p)) return false;
    ntuple_plan(n, *p, plan);
    return true;
}

template <int W>
void eval_rows(int R, const uint32_t* plan, const int32_t* w, const uint64_t* boards, const uint16_t* meta, int32_t* values,
               int64_t* sums) {
    for (int r = 0; r < R; ++r) ntuple_eval_row_host<W>(plan, w, boards, meta, (size_t)r, values, sums);
}

template <int W>
void add_rows(int R, const uint32_t* plan, uint32_t* w, const uint64_t* boards, const uint16_t* meta, const int32_t* deltas) {
    for (int r = 0; r < R; ++r) ntuple_add_row_host<W>(plan, w, boards, meta, (size_t)r, deltas[r]);
}

template <int N>
void search_n(int E, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal, int depth, const uint32_t* plan,
              const int32_t* weights, int terminal, uint32_t max_nodes, int32_t* value, int32_t* best, int32_t* move_values,
              uint8_t* status, uint64_t* nodes) {
    constexpr int W = Geo<N>::W, NN = N * N;
    for (int e = 0; e < E; ++e)
        status[e] = (uint8_t)ntuple_search_board_host<N>(boards + (size_t)e * 2 * W, boards + (size_t)e * 2 * W + W,
                                                         legal + (size_t)e * W, meta[e], depth, plan, weights, terminal,
                                                         max_nodes, value + e, best + e, move_values + (size_t)e * NN,
                                                         nodes + e);
}

}  // namespace

// n_weights + 1, or 0 for parameters out of range
extern "C" uint64_t host_ntuple_weight_count(int n, const NtupleParams* p) {
    if (!p || ntuple_check(n, p)) return 0;
    return (uint64_t)ntuple_n_weights(*p) + 1u;
}

// the plan's bytes into out (capacity bytes); returns their number, 0 for parameters out of range or a short buffer
extern "C" uint64_t host_ntuple_plan(int n, const NtupleParams* p, void* out, uint64_t capacity) {
    uint32_t plan[PLAN_WORDS];
    if (!make_plan(n, p, plan)) return 0;
    const uint64_t bytes = ntuple_plan_bytes(*p);
    if (capacity < bytes) return 0;
    memcpy(out, plan, bytes);
    return bytes;
}

// 0, 1 for arguments out of range (nothing is written)
extern "C" int host_ntuple_eval(int n, int R, const NtupleParams* p, const int32_t* weights, const uint64_t* boards,
                                const uint16_t* meta, int32_t* values, int64_t* sums) {
    uint32_t plan[PLAN_WORDS];
    if (!make_plan(n, p, plan) || R < 0 || !weights || !boards || !meta || !values) return 1;
    switch ((n * n + 63) / 64) {
        case 1: eval_rows<1>(R, plan, weights, boards, meta, values, sums); break;
        case 2: eval_rows<2>(R, plan, weights, boards, meta, values, sums); break;
        case 3: eval_rows<3>(R, plan, weights, boards, meta, values, sums); break;
        default: eval_rows<4>(R, plan, weights, boards, meta, values, sums); break;
    }
    return 0;
}

// oth_ntuple_update: every delta from the old weights first, then the additions
extern "C" int host_ntuple_update(int n, int R, const NtupleParams* p, int32_t* weights, const uint64_t* boards,
                                  const uint16_t* meta, const int32_t* targets, int32_t rate, int32_t rate_shift,
                                  int32_t* deltas) {
    uint32_t plan[PLAN_WORDS];
    if (!make_plan(n, p, plan) || R < 0 || !weights || !boards || !meta || !targets || !deltas || rate < 0 ||
        rate > NTUPLE_MAX_RATE || rate_shift < 0 || rate_shift > NTUPLE_MAX_RATE_SHIFT)
        return 1;
    if (host_ntuple_eval(n, R, p, weights, boards, meta, deltas, nullptr)) return 1;  // (the values, for a moment)
    for (int r = 0; r < R; ++r) deltas[r] = ntuple_delta(targets[r], deltas[r], rate, rate_shift);
    uint32_t* w = reinterpret_cast<uint32_t*>(weights);
    switch ((n * n + 63) / 64) {
        case 1: add_rows<1>(R, plan, w, boards, meta, deltas); break;
        case 2: add_rows<2>(R, plan, w, boards, meta, deltas); break;
        case 3: add_rows<3>(R, plan, w, boards, meta, deltas); break;
        default: add_rows<4>(R, plan, w, boards, meta, deltas); break;
    }
    return 0;
}

extern "C" int host_search_ntuple(int n, int E, const uint64_t* boards, const uint16_t* meta, const uint64_t* legal,
                                  int depth, const NtupleParams* p, const int32_t* weights, int terminal,
                                  uint64_t max_nodes, int32_t* value, int32_t* best, int32_t* move_values,
                                  uint8_t* status, uint64_t* nodes) {
    uint32_t plan[PLAN_WORDS];
    if (!make_plan(n, p, plan) || !weights || depth < 1 || depth > SEARCH_MAX_DEPTH || terminal < 1 || terminal > 32767 ||
        max_nodes < 1 || max_nodes > 0xffffffffull)
        return 1;
    const uint32_t mn = (uint32_t)max_nodes;
    switch (n) {
#define CASE(K)                                                                                                      \
    case K:                                                                                                          \
        search_n<K>(E, boards, meta, legal, depth, plan, weights, terminal, mn, value, best, move_values, status, nodes); \
        break;
#ifdef NTUPLE_SAN_MAIN  // the sanitizer program's sizes only: one-, two- and four-word frames, a shorter build
        CASE(4) CASE(8) CASE(10) CASE(16)
#else
        CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#endif
#undef CASE
        default: return 1;
    }
    return 0;
}
