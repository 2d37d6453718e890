// Micro-benchmark: what a lone wave (one per SIMD, the 65,536-board configs) pays
// for the select forms the play kernels' ply holds -- v_cndmask_b32 on an SGPR
// pair or on VCC, alone and behind the v_cmp that feeds it, the exec-masked
// region's compare / saveexec / branch / restore -- and for the mask forms that
// can replace them, in the explicit-register harness of ubench_valu3.hip (16
// independent chains, 128 and 256 ops per loop iteration); then the two complete
// pick sequences, select64_tab with compares and selects (the body before this
// tool, kept here) and the compare-free select64_tab of bitboard.hpp, each fed
// by its ds_read_u8 from the staged 2-KiB table.  Build + run on the GPU box:
//   hipcc --offload-arch=gfx950 -O3 -o tools/ubench_select tools/ubench_select.hip && tools/ubench_select
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../gymothelloenv_amd/csrc/bitboard.hpp"

#define CLOB                                                                                                          \
    "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23",    \
        "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38",     \
        "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53",     \
        "v54", "v55", "s40", "s41", "s42", "s43", "s44", "s45"

// every VGPR of the harness = the lane's seed; s40 a constant, s[42:43] a mask of alternating lanes
#define INIT                                                                                                          \
    "v_mov_b32 v8, %1\n v_mov_b32 v9, %1\n v_mov_b32 v10, %1\n v_mov_b32 v11, %1\n v_mov_b32 v12, %1\n"              \
    " v_mov_b32 v13, %1\n v_mov_b32 v14, %1\n v_mov_b32 v15, %1\n v_mov_b32 v16, %1\n v_mov_b32 v17, %1\n"           \
    " v_mov_b32 v18, %1\n v_mov_b32 v19, %1\n v_mov_b32 v20, %1\n v_mov_b32 v21, %1\n v_mov_b32 v22, %1\n"           \
    " v_mov_b32 v23, %1\n v_mov_b32 v24, %1\n v_mov_b32 v25, %1\n v_mov_b32 v26, %1\n v_mov_b32 v27, %1\n"           \
    " v_mov_b32 v28, %1\n v_mov_b32 v29, %1\n v_mov_b32 v30, %1\n v_mov_b32 v31, %1\n v_mov_b32 v32, %1\n"           \
    " v_mov_b32 v33, %1\n v_mov_b32 v34, %1\n v_mov_b32 v35, %1\n v_mov_b32 v36, %1\n v_mov_b32 v37, %1\n"           \
    " v_mov_b32 v38, %1\n v_mov_b32 v39, %1\n v_mov_b32 v40, %1\n v_mov_b32 v41, %1\n v_mov_b32 v42, %1\n"           \
    " v_mov_b32 v43, %1\n v_mov_b32 v44, %1\n v_mov_b32 v45, %1\n v_mov_b32 v46, %1\n v_mov_b32 v47, %1\n"           \
    " v_mov_b32 v48, %1\n v_mov_b32 v49, %1\n v_mov_b32 v50, %1\n v_mov_b32 v51, %1\n v_mov_b32 v52, %1\n"           \
    " v_mov_b32 v53, %1\n v_mov_b32 v54, %1\n v_mov_b32 v55, %1\n s_mov_b32 s40, 0x5555\n s_mov_b32 s41, 0\n"        \
    " s_mov_b32 s42, 0x55555555\n s_mov_b32 s43, 0x55555555\n"
#define INIT_VCC " s_mov_b64 vcc, s[42:43]\n"
#define INIT_VCC_VALU " v_cmp_le_i32_e32 vcc, v8, v49\n"

#define X8(b) b b b b b b b b
#define X16(b) X8(b) X8(b)
// a kernel whose loop body is `rep(blk)`; the variadic tail: further clobbers ("vcc", "scc") where the body or
// INIT writes them
#define KERNEL(name, init, rep, blk, ...)                                                                             \
    __global__ void name(uint32_t* out, int iters) {                                                                 \
        uint32_t r;                                                                                                   \
        const uint32_t seed = threadIdx.x * 2654435761u + 1u;                                                        \
        asm volatile(init : "=v"(r) : "v"(seed) : CLOB, ##__VA_ARGS__);                                              \
        for (int i = 0; i < iters; ++i) asm volatile(rep(blk) : : : CLOB, ##__VA_ARGS__);                            \
        asm volatile("v_xor_b32 %0, v8, v12\n v_or3_b32 %0, %0, v16, v20\n v_or3_b32 %0, %0, v9, v10\n"            \
                     " v_or3_b32 %0, %0, v11, v13\n v_or3_b32 %0, %0, v14, v15\n v_or3_b32 %0, %0, v17, v18\n"     \
                     " v_or3_b32 %0, %0, v19, v21\n v_or3_b32 %0, %0, v22, v23\n v_or3_b32 %0, %0, v28, v28"       \
                     : "=v"(r) : : CLOB, ##__VA_ARGS__);                                                             \
        out[blockIdx.x * blockDim.x + threadIdx.x] = r;                                                               \
    }
// both loop lengths of one block
#define K2(name, init, blk, ...)                                                                                      \
    KERNEL(name##_a, init, X8, blk, ##__VA_ARGS__)                                                                    \
    KERNEL(name##_b, init, X16, blk, ##__VA_ARGS__)

#define S(x) #x
#define G16(f) f(8) f(9) f(10) f(11) f(12) f(13) f(14) f(15) f(16) f(17) f(18) f(19) f(20) f(21) f(22) f(23)
#define G8(f) f(8) f(9) f(10) f(11) f(12) f(13) f(14) f(15)
// 16-op blocks
#define AND(d) "v_and_b32 v" S(d) ", v" S(d) ", v49\n"
#define CND64(d) "v_cndmask_b32_e64 v" S(d) ", v" S(d) ", v49, s[42:43]\n"
#define CMPCND64(d) "v_cmp_le_i32_e64 s[42:43], v" S(d) ", v49\n v_cndmask_b32_e64 v" S(d) ", v" S(d) ", v50, s[42:43]\n"
#define CMP3CND64(a, b, c)                                                                                            \
    "v_cmp_le_i32_e64 s[42:43], v" S(a) ", v49\n v_cndmask_b32_e64 v" S(a) ", v" S(a) ", v50, s[42:43]\n"            \
    " v_cndmask_b32_e64 v" S(b) ", v" S(b) ", v50, s[42:43]\n v_cndmask_b32_e64 v" S(c) ", v" S(c) ", v50, s[42:43]\n"
#define CND32(d) "v_cndmask_b32_e32 v" S(d) ", v" S(d) ", v49, vcc\n"
#define CMP1CND32(d) "v_cmp_le_i32_e32 vcc, v" S(d) ", v49\n"
#define CMPCND32(d) "v_cmp_le_i32_e32 vcc, v" S(d) ", v49\n v_cndmask_b32_e32 v" S(d) ", v" S(d) ", v50, vcc\n"
#define SUBASHRB3(d)                                                                                                  \
    "v_sub_u32 v" S(d) ", v" S(d) ", v49\n v_ashrrev_i32 v" S(d) ", 31, v" S(d) "\n"                                 \
    " v_bitop3_b32 v" S(d) ", v" S(d) ", v49, v50 bitop3:0xca\n"
#define BFEI(d) "v_bfe_i32 v" S(d) ", v" S(d) ", 31, 1\n"
#define ASHR(d) "v_ashrrev_i32 v" S(d) ", 31, v" S(d) "\n"
#define MAX3(d) "v_max3_u32 v" S(d) ", v" S(d) ", v49, v50\n"
#define PERM(d) "v_perm_b32 v" S(d) ", v" S(d) ", v49, s40\n"
#define BCNT(d) "v_bcnt_u32_b32 v" S(d) ", v" S(d) ", v49\n"
#define B3(d) "v_bitop3_b32 v" S(d) ", v" S(d) ", v49, v50 bitop3:0xca\n"
// the ply's exec-masked region around one v_and: compare -> saveexec -> execz branch -> restore.
// Every VGPR holds the lane's seed, so eq is true on every lane (branch not taken) and ne on none (taken)
#define REGION(cmp)                                                                                                   \
    "v_cmp_" cmp "_u64_e64 s[42:43], v[24:25], v[26:27]\n s_and_saveexec_b64 s[44:45], s[42:43]\n"                   \
    " s_cbranch_execz 1f\n v_and_b32 v28, v28, v49\n1:\n s_or_b64 exec, exec, s[44:45]\n"

K2(k_and, INIT, G16(AND))
K2(k_cnd64, INIT, G16(CND64))
K2(k_cmpcnd64, INIT, G8(CMPCND64))
K2(k_cmp3cnd64, INIT, CMP3CND64(8, 9, 10) CMP3CND64(11, 12, 13) CMP3CND64(14, 15, 16) CMP3CND64(17, 18, 19))
K2(k_cnd32_once, INIT INIT_VCC, G16(CND32), "vcc")
K2(k_cnd32_once_valu, INIT INIT_VCC_VALU, G16(CND32), "vcc")
K2(k_cnd32_never, INIT, G16(CND32))  // ubench_valu3's row: VCC neither written nor declared
K2(k_cmp15cnd32, INIT, CMP1CND32(8) CND32(9) CND32(10) CND32(11) CND32(12) CND32(13) CND32(14) CND32(15) CND32(16) CND32(17) CND32(18) CND32(19) CND32(20) CND32(21) CND32(22) CND32(23), "vcc")
K2(k_cmpcnd32, INIT, G8(CMPCND32), "vcc")
K2(k_subashrb3, INIT, SUBASHRB3(8) SUBASHRB3(9) SUBASHRB3(10) SUBASHRB3(11) SUBASHRB3(12) SUBASHRB3(13) SUBASHRB3(14) SUBASHRB3(15))
K2(k_bfei, INIT, G16(BFEI))
K2(k_ashr, INIT, G16(ASHR))
K2(k_max3, INIT, G16(MAX3))
K2(k_perm, INIT, G16(PERM))
K2(k_bcnt, INIT, G16(BCNT))
K2(k_b3, INIT, G16(B3))
K2(k_region_not, INIT, G16(AND) REGION("eq"), "scc")
K2(k_region_taken, INIT, G16(AND) REGION("ne"), "scc")
// the region's parts, each beside 16 v_and
#define CMP64 "v_cmp_eq_u64_e64 s[42:43], v[24:25], v[26:27]\n"
#define SAVEX "s_and_saveexec_b64 s[44:45], s[42:43]\n"
#define RESTX "s_or_b64 exec, exec, s[44:45]\n"
#define AND28 "v_and_b32 v28, v28, v49\n"
#define AND8B(d) "v_and_b32 v" S(d) ", v" S(d) ", v49\n"
#define G8B(f) f(16) f(17) f(18) f(19) f(20) f(21) f(22) f(23)
K2(k_part_cmp, INIT, G16(AND) CMP64)
K2(k_part_exec, INIT, G16(AND) SAVEX AND28 RESTX, "scc")
K2(k_part_cmp_exec, INIT, G16(AND) CMP64 SAVEX AND28 RESTX, "scc")
K2(k_part_branch, INIT, G16(AND) "s_cbranch_execz 1f\n1:\n")
K2(k_region_spaced, INIT, G8(AND) CMP64 G8B(AND8B) SAVEX "s_cbranch_execz 1f\n" AND28 "1:\n" RESTX, "scc")
#define CND64VCC(d) "v_cndmask_b32_e64 v" S(d) ", v" S(d) ", v49, vcc\n"
K2(k_cnd64_vcc_once, INIT INIT_VCC, G16(CND64VCC), "vcc")

// select64_tab as it was with compares and selects (bitboard.hpp before the mask form)
__device__ __forceinline__ int select64_tab_cmp(uint64_t x, int k, const uint8_t* sel8) {
    using oth::popc64;
    const uint32_t lo = (uint32_t)x;
    const int c = popc64(lo);
    const bool up = k >= c;
    const uint32_t v = up ? (uint32_t)(x >> 32) : lo;
    const int kk = up ? k - c : k;
    const int q1 = popc64(v & 0xFFu), q2 = popc64(v & 0xFFFFu), q3 = popc64(v & 0xFFFFFFu);
    const bool m1 = q1 <= kk, m2 = q2 <= kk, m3 = q3 <= kk;
    const int b = (int)m1 + (int)m2 + (int)m3;
    const int qb = m3 ? q3 : (m2 ? q2 : (m1 ? q1 : 0));
    const uint32_t byte = __builtin_amdgcn_ubfe(v, 8u * (uint32_t)b, 8u);
    return (up ? 32 : 0) + 8 * b + sel8[8 * byte + (uint32_t)(kk - qb)];
}

// PICKS dependent picks per iteration, as in a ply: the draw scaled to the word's
// count, the pick, the next draw and word from the picked square (the word rotated:
// nothing of the pick is loop-invariant)
constexpr int PICKS = 8;
template <bool MASKS>
__global__ void k_pick(uint32_t* out, int iters) {
    __shared__ __attribute__((aligned(16))) uint64_t lds_sel[256];
    lds_sel[threadIdx.x] = oth::sel8_word(threadIdx.x);
    __syncthreads();
    const uint8_t* sel8 = reinterpret_cast<const uint8_t*>(lds_sel);
    uint32_t u = threadIdx.x * 2654435761u + 1u, acc = 0;
    uint64_t L = ((uint64_t)(u * 0x85EBCA6Bu) << 32 | u * 0xC2B2AE35u) | 1ull;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int j = 0; j < PICKS; ++j) {
            const int k = oth::scale_index(u, oth::popc64(L));
            const int a = MASKS ? oth::select64_tab(L, k, sel8) : select64_tab_cmp(L, k, sel8);
            acc += (uint32_t)a;
            u = __builtin_rotateleft32(u, 5) ^ (uint32_t)a;
            L = (L << 1) | (L >> 63);
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

typedef void (*K)(uint32_t*, int);

static float run(K k, int waves_per_simd, int iters, uint32_t* buf) {
    const int blocks = 256 * waves_per_simd;  // 256-thread blocks: 4 waves each = 1 per SIMD of a CU
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, buf, iters);
    (void)hipEventRecord(a, 0);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, buf, iters);
    (void)hipEventRecord(b, 0);
    (void)hipEventSynchronize(b);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return ms;
}

int main() {
    uint32_t* buf;
    if (hipMalloc(&buf, 256 * 16 * 256 * 4) != hipSuccess) return 1;
    const int iters = 2000;
    struct T {
        const char* name;
        K ka, kb;
        int units;  // per 16-op block (loop bodies: 8 and 16 blocks)
        int ops;    // instructions per unit
    } ks[] = {
        {"v_and_b32 (v, v)", k_and_a, k_and_b, 16, 1},
        {"v_cndmask_b32_e64 (v, v, s[a:b] long-lived)", k_cnd64_a, k_cnd64_b, 16, 1},
        {"v_cmp_le_i32_e64 s[a:b] -> v_cndmask_b32_e64 (per pair)", k_cmpcnd64_a, k_cmpcnd64_b, 8, 2},
        {"v_cmp_le_i32_e64 s[a:b] -> 3 v_cndmask_b32_e64 (per four)", k_cmp3cnd64_a, k_cmp3cnd64_b, 4, 4},
        {"v_cndmask_b32_e32 (v, v, vcc written once before the loop by s_mov_b64)", k_cnd32_once_a, k_cnd32_once_b, 16, 1},
        {"v_cndmask_b32_e32 (v, v, vcc written once before the loop by a v_cmp)", k_cnd32_once_valu_a, k_cnd32_once_valu_b,
         16, 1},
        {"v_cndmask_b32_e32 (v, v, vcc never written)", k_cnd32_never_a, k_cnd32_never_b, 16, 1},
        {"v_cmp_le_i32_e32 vcc + 15 v_cndmask_b32_e32 (per instruction)", k_cmp15cnd32_a, k_cmp15cnd32_b, 16, 1},
        {"v_cmp_le_i32_e32 vcc -> v_cndmask_b32_e32 (per pair)", k_cmpcnd32_a, k_cmpcnd32_b, 8, 2},
        {"v_sub_u32 -> v_ashrrev_i32 31 -> v_bitop3_b32 0xCA (per three)", k_subashrb3_a, k_subashrb3_b, 8, 3},
        {"v_bfe_i32 (v, 31, 1)", k_bfei_a, k_bfei_b, 16, 1},
        {"v_ashrrev_i32 (31, v)", k_ashr_a, k_ashr_b, 16, 1},
        {"v_max3_u32 (v, v, v)", k_max3_a, k_max3_b, 16, 1},
        {"v_perm_b32 (v, v, s)", k_perm_a, k_perm_b, 16, 1},
        {"v_bcnt_u32_b32 (v, v)", k_bcnt_a, k_bcnt_b, 16, 1},
        {"v_bitop3_b32 0xCA (v, v, v)", k_b3_a, k_b3_b, 16, 1},
        {"v_cndmask_b32_e64 (v, v, vcc written once before the loop by s_mov_b64)", k_cnd64_vcc_once_a, k_cnd64_vcc_once_b,
         16, 1},
        {"16 v_and_b32 + v_cmp_eq_u64_e64", k_part_cmp_a, k_part_cmp_b, 1, 17},
        {"16 v_and_b32 + s_and_saveexec_b64 (long-lived mask) / v_and / s_or_b64 exec", k_part_exec_a, k_part_exec_b, 1, 19},
        {"16 v_and_b32 + v_cmp_eq_u64_e64 / s_and_saveexec_b64 / v_and / s_or_b64 exec (no branch)", k_part_cmp_exec_a,
         k_part_cmp_exec_b, 1, 20},
        {"16 v_and_b32 + s_cbranch_execz not taken", k_part_branch_a, k_part_branch_b, 1, 17},
        {"8 v_and_b32 + v_cmp_eq_u64_e64 + 8 v_and_b32 + s_and_saveexec_b64 / s_cbranch_execz not taken / v_and / s_or_b64 exec",
         k_region_spaced_a, k_region_spaced_b, 1, 22},
        {"16 v_and_b32 + v_cmp_eq_u64_e64 / s_and_saveexec_b64 / s_cbranch_execz not taken / v_and / s_or_b64 exec",
         k_region_not_a, k_region_not_b, 1, 22},
        {"16 v_and_b32 + v_cmp_ne_u64_e64 / s_and_saveexec_b64 / s_cbranch_execz taken / s_or_b64 exec",
         k_region_taken_a, k_region_taken_b, 1, 21},
    };
    printf("{\"clock_note\": \"cycles assume 2.4 GHz; per wave, of its SIMD's time\", \"results\": [\n");
    bool first = true;
    for (auto& t : ks)
        for (int blocks16 : {8, 16})
            for (int w : {1, 2}) {
                const float ms = run(blocks16 == 8 ? t.ka : t.kb, w, iters, buf);
                const double ns = ms * 1e6 / ((double)iters * blocks16 * t.units);
                printf("%s{\"form\": \"%s\", \"instructions_per_unit\": %d, \"ops_per_iteration\": %d, "
                       "\"waves_per_simd\": %d, \"cycles_per_unit\": %.3f}",
                       first ? "" : ",\n", t.name, t.ops, blocks16 * t.units * t.ops, w, ns / w * 2.4);
                first = false;
            }
    struct P {
        const char* name;
        K k;
    } ps[] = {{"pick: select64_tab with compares and selects + ds_read_u8", k_pick<false>},
              {"pick: select64_tab by masks (bitboard.hpp) + ds_read_u8", k_pick<true>}};
    for (auto& p : ps)
        for (int w : {1, 2}) {
            const float ms = run(p.k, w, iters, buf);
            printf(",\n{\"form\": \"%s\", \"picks_per_iteration\": %d, \"waves_per_simd\": %d, \"cycles_per_pick\": %.3f}",
                   p.name, PICKS, w, ms * 1e6 / ((double)iters * PICKS) / w * 2.4);
        }
    printf("\n]}\n");
    (void)hipFree(buf);
    return 0;
}
