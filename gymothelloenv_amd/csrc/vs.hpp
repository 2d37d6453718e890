// vs.hpp -- OthelloEnv on the device (oth_reset_vs / oth_step_vs): the embedded
// opponent's replies around the protagonist's ply, any board size and policy.
#pragma once
#include "policy.hpp"

namespace oth_dev {

// ---------------------------------------------------------------------------
// OthelloEnv semantics on the device (othello.py:151-200): the protagonist
// steps with the caller's action, then the embedded opponent (random or greedy,
// on device) replies until it is the protagonist's turn again; the reward of
// a game the opponent's ply ends is negated (:200).  Random-opening plies
// (SimpleOthelloEnv / OthelloEnv rand_step_cnt, :179-182, :191-194) replace
// both sides' moves by random ones; the opponent's reply inside reset() uses
// the policy directly (:165-174).  Draws: ply j of call c uses
// action_draw(seed, id, c * 256 + j).
// ---------------------------------------------------------------------------
constexpr uint64_t VS_PLIES_PER_CALL = 256;

template <int N, int POLICY>
__device__ __forceinline__ void opponent_reply(Lane<N>& s, bool prot_white, bool openings, uint32_t flags,
                                               const Rng& rng, uint32_t id, uint64_t gbase, uint32_t& j, int& r,
                                               int& d, int& win) {
    const Solo<N> eng(0, nullptr);
    while (!(s.meta & M_TERMINATED) && (((s.meta & M_TURN_WHITE) != 0) != prot_white)) {
        const uint32_t rl = s.meta >> M_RAND_SHIFT;
        const uint64_t g = gbase + j++;  // ply j of the call
        int a;
        if (POLICY == OTH_POLICY_RANDOM || (openings && rl > 0)) {
            a = random_action<N>(s, action_draw(rng.seed, id, g));
        } else {
            a = policy_action<N, POLICY>(s, eng, rng.depth);
        }
        if (openings && rl > 0) s.meta -= 1u << M_RAND_SHIFT;
        step_lane<N>(s, a, flags, r, d, win, eng);
    }
}

template <int N, int POLICY>
__device__ __forceinline__ void reset_vs_lane(Lane<N>& s, bool prot_white, uint32_t flags, const Rng& rng,
                                              uint32_t id, uint64_t call, uint32_t purpose, uint32_t& j) {
    reset_lane<N>(s, rng.seed, id, call, purpose, rng.init_rand);
    int r, d, win;
    opponent_reply<N, POLICY>(s, prot_white, false, flags, rng, id, call * VS_PLIES_PER_CALL, j, r, d, win);
}

template <int N, int POLICY>
__global__ __launch_bounds__(BLOCK) void k_reset_vs(uint64_t* __restrict__ boards, uint16_t* __restrict__ meta,
                                                    uint64_t* __restrict__ legal, int E, uint32_t flags,
                                                    const int8_t* __restrict__ prot, const uint8_t* __restrict__ mask,
                                                    Rng rng, uint64_t call) {
    call += *rng.ply_off;  // graph-region offset (oth_graph_end); 0 eagerly
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= E) return;
    if (mask && !mask[e]) return;
    const bool pw = prot ? prot[e] == WHITE_DISK : true;
    Lane<N> s;
    uint32_t j = 0;
    reset_vs_lane<N, POLICY>(s, pw, flags, rng, rng.id_base + (uint32_t)e, call, RNG_OPENING_RESET, j);
    store_lane<N>(s, boards, meta, legal, e);
}

template <int N, int POLICY>
__global__ __launch_bounds__(BLOCK) void k_step_vs(uint64_t* __restrict__ boards, uint16_t* __restrict__ meta,
                                                   uint64_t* __restrict__ legal, int E, uint32_t flags,
                                                   const int32_t* __restrict__ actions, const int8_t* __restrict__ prot,
                                                   int32_t* __restrict__ rewards, uint8_t* __restrict__ dones,
                                                   int32_t* __restrict__ plies_out,
                                                   unsigned long long* __restrict__ wdl,
                                                   unsigned long long* __restrict__ wdl_vs, Rng rng, uint64_t call) {
    call += *rng.ply_off;  // graph-region offset (oth_graph_end); 0 eagerly
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t cb = 0, cd = 0, cw = 0, pw_n = 0, pd_n = 0, pl_n = 0;
    if (e < E) {
        const uint32_t id = rng.id_base + (uint32_t)e;
        const bool pw = prot ? prot[e] == WHITE_DISK : true;
        const uint64_t gbase = call * VS_PLIES_PER_CALL;
        Lane<N> s;
        load_lane<N>(s, boards, meta, legal, e);
        uint32_t j = 0;
        int r = 0, d = 1, win = NO_DISK, plies = 0;
        if (!(s.meta & M_TERMINATED)) {
            const Solo<N> eng(0, nullptr);
            d = 0;
            // the protagonist must be to move (OthelloEnv.step asserts it, othello.py:177);
            // if not, the opponent replies first, as OthelloEnv.reset does
            opponent_reply<N, POLICY>(s, pw, true, flags, rng, id, gbase, j, r, d, win);
            if (!(s.meta & M_TERMINATED)) {
                int a = actions[e];
                const uint32_t rl = s.meta >> M_RAND_SHIFT;
                const uint64_t g = gbase + j++;
                if (rl > 0) {  // opening ply: the protagonist's action is replaced too (:179-182)
                    a = random_action<N>(s, action_draw(rng.seed, id, g));
                    s.meta -= 1u << M_RAND_SHIFT;
                }
                step_lane<N>(s, a, flags, r, d, win, eng);
                if (!d) {
                    opponent_reply<N, POLICY>(s, pw, true, flags, rng, id, gbase, j, r, d, win);
                    r = -r;  // :200
                }
            } else {
                r = -r;
            }
            plies = (int)j;
            if (d) {
                cb = win == BLACK_DISK;
                cd = win == NO_DISK;
                cw = win == WHITE_DISK;
                // the harnesses' count from the protagonist's final reward (run.py:100-130:
                // its sign is the protagonist's result in both reward modes)
                const int pcol = pw ? WHITE_DISK : BLACK_DISK;
                pw_n = win == pcol;
                pd_n = win == NO_DISK;
                pl_n = win == -pcol;
                if (flags & OTH_AUTO_RESET) reset_vs_lane<N, POLICY>(s, pw, flags, rng, id, call, RNG_OPENING_AUTO, j);
            }
        }
        store_lane<N>(s, boards, meta, legal, e);
        if (rewards) rewards[e] = r;
        if (dones) dones[e] = (uint8_t)d;
        if (plies_out) plies_out[e] = plies;
    }
    tally(wdl, cb, cd, cw);
    tally(wdl_vs, pw_n, pd_n, pl_n);
}

}  // namespace oth_dev
