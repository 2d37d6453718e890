// play.hpp -- oth_step_policy: k_play (any policy, any engine) and the fast
// random / greedy play kernels k_play_rand (one-word boards) and k_play_rand_w
// (multi-word boards) with their plies play_rand_fast(_w).
#pragma once
#include "policy.hpp"

namespace oth_dev {

// oth_step_policy: `plies` plies of on-device play with the board kept in
// registers between plies; per-ply outputs stored [ply][E].  One lane per board.
// REC: all three per-ply outputs requested (stores without per-pointer branches,
// so the ply's tail stays one basic block the scheduler can interleave).
template <int N, int POLICY, typename Eng, bool REC>
__global__ __launch_bounds__(BLOCK) void k_play(uint64_t* __restrict__ boards, uint16_t* __restrict__ meta,
                                                uint64_t* __restrict__ legal, int E, uint32_t flags, int plies,
                                                int32_t* __restrict__ actions, int32_t* __restrict__ rewards,
                                                uint8_t* __restrict__ dones, unsigned long long* __restrict__ wdl,
                                                Rng rng, uint64_t ply0) {
    ply0 += *rng.ply_off;  // graph-region offset (oth_graph_end); 0 eagerly
    __shared__ __attribute__((aligned(16))) uint64_t lds_rays[Eng::RAY_WORDS > 0 ? Eng::RAY_WORDS : 1];
    if constexpr (is_fills_w<Eng>::value) Eng::fill(lds_rays);
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    const Eng eng(0, lds_rays);
    // always true (one lane per board).  The guard stays on the stores below: without it
    // the same instructions come out in another block order in most instantiations
    // (DESIGN.md section 5), and they have no benchmark line each to measure that against
    const bool lead = eng.leader();
    uint32_t cb = 0, cd = 0, cw = 0;
    if (e < E) {
        const uint32_t id = rng.id_base + (uint32_t)e;
        Lane<N> s;
        load_lane<N>(s, boards, meta, legal, e);
        eng.prime(s);
        int32_t* act_p = actions + e;
        int32_t* rew_p = rewards + e;
        uint8_t* done_p = dones + e;
        // one ply; u_rand = the random policy's 32-bit draw for this ply
        auto ply = [&](int p, uint32_t u_rand) __attribute__((always_inline)) {
            const uint64_t g = ply0 + (uint64_t)p;
            const size_t o = (size_t)p * (size_t)E + (size_t)e;
            int a = -1, r = 0, d = 1, win = NO_DISK;
            if (!(s.meta & M_TERMINATED)) {
                const uint32_t rl = s.meta >> M_RAND_SHIFT;
                if (POLICY == OTH_POLICY_RANDOM || rl > 0) {
                    const uint32_t u = POLICY == OTH_POLICY_RANDOM ? u_rand : action_draw(rng.seed, id, g);
                    a = random_action<N>(s, u);
                    if (rl > 0) s.meta -= 1u << M_RAND_SHIFT;
                } else {
                    a = policy_action<N, POLICY>(s, eng, rng.depth);
                }
                step_lane<N, Eng, true>(s, a, flags, r, d, win, eng);  // a: a pick from s.legal
                if (d) {
                    cb += win == BLACK_DISK;
                    cd += win == NO_DISK;
                    cw += win == WHITE_DISK;
                    if (flags & OTH_AUTO_RESET) {
                        reset_lane<N>(s, rng.seed, id, g, RNG_OPENING_AUTO, rng.init_rand);
                        eng.prime(s);
                    }
                }
            }
            if (lead) {
                if constexpr (REC) {  // running pointers: one 64-bit add each per ply
                    *act_p = a;
                    *rew_p = r;
                    *done_p = (uint8_t)d;
                    act_p += E;
                    rew_p += E;
                    done_p += E;
                } else {
                    if (actions) actions[o] = a;
                    if (rewards) rewards[o] = r;
                    if (dones) dones[o] = (uint8_t)d;
                }
            }
        };
        if constexpr (POLICY == OTH_POLICY_RANDOM) {
            // Philox block g/4 gives plies 4k..4k+3 their words x, y, z, w: four
            // plies unrolled per block once g is 4-aligned (g is uniform, so
            // these branches are scalar); single plies before and after
            int p = 0;
            while (p < plies) {
                const uint64_t g = ply0 + (uint64_t)p;
                const U4 d4 = philox4(rng.seed, id, g >> 2, RNG_ACTION);
                if ((g & 3) == 0 && p + 4 <= plies) {
                    ply(p, d4.x);
                    ply(p + 1, d4.y);
                    ply(p + 2, d4.z);
                    ply(p + 3, d4.w);
                    p += 4;
                } else {
                    ply(p, pick4(d4, (uint32_t)(g & 3)));
                    ++p;
                }
            }
        } else {  // scripted policies draw only on random-opening plies (action_draw inside ply)
            for (int p = 0; p < plies; ++p) ply(p, 0u);
        }
        if (lead) store_lane<N>(s, boards, meta, legal, e);
    }
    tally(wdl, cb, cd, cw);
}

// k_play_rand: oth_step_policy(RANDOM) on one-word boards with auto-reset and
// every per-ply output stored -- the benchmark configuration -- with the
// same results as k_play<N, RANDOM, Fills<N>, true>, restructured for one
// wave per SIMD, where every VALU instruction of every path a lane of the
// wave takes is paid by the whole wave:
//   * the board is held as (mover, opponent) plus the side-to-move bit, so a
//     ply swaps two words once instead of selecting mover / opponent from
//     (black, white) and writing them back (othello.py:412-462 flips the
//     `player_turn`, not the board);
//   * with auto-reset no board is terminated at a ply's start, so there is no
//     per-ply "terminated?" branch and no branch-join copies of the carried
//     fills (a wave holding a board loaded terminated runs k_play's body);
//   * the opponent's legal scan runs unconditionally (on a full board it
//     finds nothing: no empty square); only a pass re-scans, in place.
// The random pick is always legal, so sudden death never triggers here.
// POLICY GREEDY (k_play_rand<N, GREEDY>): GreedyPolicy's move from the bit
// planes of the carried fills (simple_policies.py:69-92), a random move while
// random-opening plies remain (SimpleOthelloEnv, othello.py:60-79).
// OPEN: some board of the wave may have random-opening plies left (the
// handle's initial_rand_steps > 0, or a board loaded with some); without, the
// opening bookkeeping is compiled out.
struct NoFill {
    __device__ __forceinline__ void operator()() const {}
};


// the terminal ply's reward: the disk difference (disk_reward, othello.py:446-459)
// or the sign.  By a mask on the uniform flag: as `if (flags & ...)` the backend
// made a scalar branch of it inside the terminal block (multi-word play: one per
// ply the block runs, ~40-80 cycles to a lone wave)
__device__ __forceinline__ int term_reward(uint32_t flags, int disk, int sg) {
    const uint32_t m = 0u - (uint32_t)((flags & OTH_DISK_REWARD) != 0u);
    return (int)__builtin_amdgcn_bitop3_b32(m, (uint32_t)disk, (uint32_t)sg, 0xCA);
}

// The end of a game in play_rand_fast(_w): the mover holds pc discs and its
// opponent oc, `mover`'s turn bit says who moved.  Returns the reward (:446-459 /
// winner * player_turn) and adds the game to the tally kept as (cb, cd, cw) =
// (sum of black's signs, games, decided games), which tally_from_signs turns
// into wins / draws / wins: three adds, no selects
template <int N>
__device__ __forceinline__ int fast_terminal(int pc, int oc, uint32_t mover, uint32_t flags, uint32_t& cb,
                                             uint32_t& cd, uint32_t& cw) {
    const int df = pc - oc;
    const int sg = sign_i32(df);                                    // the mover's result
    const int r = term_reward(flags, oc == 0 ? N * N : df, sg);
    const int mw = -(int)(mover & M_TURN_WHITE);                    // 0 black, -1 white
    const int sb = (sg ^ mw) - mw;                                  // black's result
    cb += (uint32_t)sb;
    cd += 1u;
    cw += (uint32_t)__mul24(sb, sb);
    return r;
}

// black wins / draws / white wins from fast_terminal's (sum of black's signs, games, decided games)
__device__ __forceinline__ void tally_from_signs(uint32_t s, uint32_t g, uint32_t z, uint32_t& cb, uint32_t& cd,
                                                 uint32_t& cw) {
    cb += (z + s) >> 1;
    cw += (z - s) >> 1;
    cd += g - z;
}
// FILL: independent work (the next Philox block) run after the opponent's scan
// and pinned there, so that it shares the ply's first scheduling region with the
// pick, the flips and the scan
template <int N, int POLICY = OTH_POLICY_RANDOM, bool OPEN = true, typename Eng = Fills<N>, typename FILL = NoFill>
__device__ __forceinline__ void play_rand_fast(uint64_t& M, uint64_t& O, uint64_t& L, uint32_t& meta,
                                               const Eng& eng, uint32_t u, uint32_t flags, const Rng& rng,
                                               uint32_t id, uint64_t g, int& a, int& r, int& d, uint32_t& cb,
                                               uint32_t& cd, uint32_t& cw, const FILL& fill = FILL{},
                                               const uint8_t* sel8 = nullptr) {
    constexpr uint64_t BD = Geo<N>::BOARD.w[0];
    // the k-th legal square, the bit inside its byte from the 2-KiB LDS table
    auto pick = [&](uint32_t draw) __attribute__((always_inline)) {
        const int k = scale_index(draw, popc64(L));
        return select64_tab(L, k, sel8);
    };
    if constexpr (POLICY == OTH_POLICY_RANDOM) {
        a = pick(u);  // RandomPolicy (simple_policies.py:37-41); L != 0
    } else if constexpr (OPEN) {
        // a random-opening ply draws u = action_draw(seed, id, g), from the caller's block
        // both computed and selected: as two exec-masked branches the wave ran both on
        // most plies (some board of the 64 in its opening) with the pick's LDS round
        // trip exposed between them; selected, the greedy planes' independent work
        // hides it: config 3 at 65,536 boards 1.378 -> 1.318 us per ply (100-ply
        // launches), 1.744 -> 1.697 (10-ply; profiles/r06/f)
        const int ap = pick(u), ag = OneWord<N>::greedy(eng.t, L);
        a = (meta & 0xff00u) ? ap : ag;
    } else {
        a = OneWord<N>::greedy(eng.t, L);
    }
    if constexpr (OPEN) meta -= (meta & 0xff00u) ? (1u << M_RAND_SHIFT) : 0u;  // a random-opening ply used up
    const uint64_t m = 1ull << a;
    BB<1> dummy;
    dummy.w[0] = 0;
    const uint64_t f = eng.flip(dummy, dummy, a).w[0];  // update_board (othello.py:391-410)
    const uint64_t Mn = M | f | m, On = O & ~f;
    const bool full = (Mn | On) == BD;  // :425-426
    if constexpr (POLICY == OTH_POLICY_RANDOM) {
        // random play: a full board ends the game and auto-resets (othello.py:256-271)
        // before the scan, which then runs on the start position (black to move)
        // instead of the full board, where it would find nothing: the reset's
        // possible_moves and fills come from it and the terminal block holds no reset
        // moves; only a double pass (inside the pass block) resets explicitly.  8x8
        // 0.678 -> 0.675 us per ply, 6x6 -1.6 %; for greedy play it measured 3 % slower
        // (the scan waits on the full-board select), so greedy keeps the reset in the
        // terminal block (profiles/r04/g/ab_term.jsonl)
        constexpr uint64_t B0 = Start<N>::BLACK.w[0], W0 = Start<N>::WHITE.w[0];
        BB<1> pb, ob;
        pb.w[0] = full ? B0 : On;
        ob.w[0] = full ? W0 : Mn;
        uint64_t Ln = eng.legal(pb, ob).w[0];  // the next mover's possible_moves (:436), fills kept in eng.t
        fill();
        const bool pass = Ln == 0;  // never on the start position
        bool term = full;
        M = pb.w[0];
        O = ob.w[0];
        if (pass) {  // :437-440: the mover moves again (fills recomputed for the mover)
            pb.w[0] = Mn;
            ob.w[0] = On;
            Ln = eng.legal(pb, ob).w[0];
            M = Mn;
            O = On;
            if (Ln == 0) {  // nobody can move (:441-442): reset
                term = true;
                start_position<N>(M, O, Ln);
                start_position_fills<N>(eng.t);
            }
        }
        L = Ln;
        const uint32_t mover = meta;
        meta ^= pass ? 0u : M_TURN_WHITE;
        r = 0;
        d = term ? 1 : 0;
        if (term) {
            r = fast_terminal<N>(popc64(Mn), popc64(On), mover, flags, cb, cd, cw);
            meta = reset_meta(rng.seed, id, g, RNG_OPENING_AUTO, rng.init_rand);
        }
    } else {
        BB<1> pb, ob;
        pb.w[0] = On;
        ob.w[0] = Mn;
        uint64_t Ln = eng.legal(pb, ob).w[0];  // the opponent's possible_moves (:436), fills kept in eng.t
        fill();
        const bool pass = Ln == 0 && !full;
        if (pass) {  // :437-440: the mover moves again (fills recomputed for the mover)
            pb.w[0] = Mn;
            ob.w[0] = On;
            Ln = eng.legal(pb, ob).w[0];
        }
        const bool term = full || Ln == 0;  // full board or nobody can move (:441-442)
        // (M, O) := (next mover, its opponent).  Alternating the two words' roles
        // statically from ply to ply instead (no selects; a pass swapping them in its
        // own exec-masked block) measured 2.3 % slower; per-ply outputs through buffer descriptors (no 64-bit
        // address VALU) 2.3 % slower too, their descriptor SALU in the same issue stream
        // (profiles/r03/st/)
        const bool swap = !pass && !full;
        M = swap ? On : Mn;
        O = swap ? Mn : On;
        L = Ln;
        meta ^= swap ? M_TURN_WHITE : 0u;
        r = 0;
        d = term ? 1 : 0;
        if (term) {  // (meta: the mover, the turn is not passed on)
            r = fast_terminal<N>(popc64(Mn), popc64(On), meta, flags, cb, cd, cw);
            // auto-reset (othello.py:256-271): black to move from the start position
            start_position<N>(M, O, L);
            start_position_fills<N>(eng.t);
            meta = reset_meta(rng.seed, id, g, RNG_OPENING_AUTO, rng.init_rand);
        }
    }
}

// tables: the handle's tables (oth_env::tables, tables.hpp); the sel8 table,
// SEL8_AT words in, is copied into LDS by one 8-byte load per thread,
// issued with the board's loads (against building it per block: greedy 10-ply
// launches 1.85 -> 1.80 us per ply, random 100-ply 0.679 -> 0.678;
// profiles/r04/b/).  The up rays before it are not read here (Fills<N>::flip).
template <int N, int POLICY = OTH_POLICY_RANDOM>
__global__ __launch_bounds__(BLOCK) void k_play_rand(uint64_t* __restrict__ boards, uint16_t* __restrict__ meta,
                                                     uint64_t* __restrict__ legal, int E, uint32_t flags, int plies,
                                                     int32_t* __restrict__ actions, int32_t* __restrict__ rewards,
                                                     uint8_t* __restrict__ dones,
                                                     unsigned long long* __restrict__ wdl, Rng rng, uint64_t ply0,
                                                     const uint64_t* __restrict__ tables) {
    static_assert(Geo<N>::W == 1, "one-word boards");
    static_assert(BLOCK == 256, "one sel8 word a thread");
    ply0 += *rng.ply_off;  // graph-region offset (oth_graph_end); 0 eagerly
    __shared__ __attribute__((aligned(16))) uint64_t lds_sel[256];
    const uint8_t* sel8 = reinterpret_cast<const uint8_t*>(lds_sel);
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    Lane<N> s;
    const uint64_t ts = tables[SEL8_AT + threadIdx.x];
    if (e < E) load_lane<N>(s, boards, meta, legal, e);
    lds_sel[threadIdx.x] = ts;
    __syncthreads();
    uint32_t cb = 0, cd = 0, cw = 0;
    if (e < E) {
        const uint32_t id = rng.id_base + (uint32_t)e;
        const Fills<N> eng(0, nullptr);
        const bool tw0 = (s.meta & M_TURN_WHITE) != 0;
        uint64_t M = tw0 ? s.white.w[0] : s.black.w[0];
        uint64_t O = tw0 ? s.black.w[0] : s.white.w[0];
        uint64_t L = s.legal.w[0];
        uint32_t mt = s.meta & (0xff00u | M_TURN_WHITE);
        eng.prime(s);
        // a board loaded terminated stays so (k_play's semantics), and a live board
        // loaded with no possible move takes the invalid path (othello.py:417-427,
        // possible_moves == [] before a reset, :242); such a wave is rare
        // (set_state) and takes the generic loop below.  Inside the fast loop no
        // live board has L == 0: a pass re-scans, a double pass terminates and
        // auto-resets.
        const bool slow = __any((s.meta & M_TERMINATED) != 0 || L == 0);
        int32_t* act_p = actions + e;
        int32_t* rew_p = rewards + e;
        uint8_t* done_p = dones + e;
        uint32_t t0 = 0, t1 = 0, t2 = 0;  // play_rand_fast's tally (tally_from_signs)
        auto fast = [&](auto OPENC) __attribute__((always_inline)) {
        constexpr bool OPEN = decltype(OPENC)::value;
        auto ply = [&](int p, uint32_t u, const auto& fill) __attribute__((always_inline)) {
            int a, r, d;
            play_rand_fast<N, POLICY, OPEN>(M, O, L, mt, eng, u, flags, rng, id, ply0 + (uint64_t)p, a, r, d, t0, t1,
                                            t2, fill, sel8);
            // the trajectory rows are written once: streaming stores (+0.9 % at 65,536
            // boards, +0.7 % at 131,072; profiles/r03/nt/).  Row stores at a scalar
            // (SGPR) row base and a constant lane offset -- 3 VALU fewer per ply, 32 SALU
            // more per 4-ply group -- measured 0.674 -> 0.709 us per ply (the lone wave's
            // issue slots: profiles/r04/c/ab_saddr.jsonl), so the running pointers stay
            __builtin_nontemporal_store(a, act_p);
            __builtin_nontemporal_store(r, rew_p);
            __builtin_nontemporal_store((uint8_t)d, done_p);
            act_p += E;
            rew_p += E;
            done_p += E;
        };
        const NoFill nofill;
        if constexpr (POLICY != OTH_POLICY_RANDOM) {  // scripted policy: draws only on opening plies
            if constexpr (OPEN) {
                // an opening ply's draw is word g % 4 of Philox block g / 4 (action_draw's
                // value).  Plies in groups of four from a multiple of 4, as random play
                // does: the group's block computed at its start and its words taken
                // statically, instead of a per-ply test for a new block and a per-ply
                // word choice (both scalar branches, ~40-80 cycles each to a lone wave):
                // config 3 at 65,536 boards, 100-ply launches 1.315 -> 1.256-1.263 us per
                // ply (profiles/r06/j, k).  (The auto-reset's opening-length draw in block form
                // measured 3-4 % slower: a wave's greedy games run almost in step, so
                // few plies see a game end, profiles/r04/oblk/.)
                int p = 0;
                // plies [p, q) inside one group: its block once, the words by pick4
                auto partial = [&](int q) __attribute__((always_inline)) {
                    const U4 blk = philox4(rng.seed, id, (ply0 + (uint64_t)p) >> 2, RNG_ACTION);
                    for (; p < q; ++p) ply(p, pick4(blk, (uint32_t)((ply0 + (uint64_t)p) & 3)), nofill);
                };
                const int head = (int)((4u - (uint32_t)(ply0 & 3)) & 3u);
                if (head > 0) partial(head < plies ? head : plies);
                while (p + 4 <= plies) {
                    const U4 blk = philox4(rng.seed, id, (ply0 + (uint64_t)p) >> 2, RNG_ACTION);
                    ply(p, blk.x, nofill);
                    ply(p + 1, blk.y, nofill);
                    ply(p + 2, blk.z, nofill);
                    ply(p + 3, blk.w, nofill);
                    p += 4;
                }
                if (p < plies) partial(plies);
            } else {
                for (int p = 0; p < plies; ++p) ply(p, 0u, nofill);
            }
            return;
        }
        int p = 0;
            // Philox block g/4 serves plies 4k..4k+3 (g uniform: scalar branches).
            // The next block is computed in the current group's first ply, after its
            // opponent scan and pinned there (FILL), where its independent VALU
            // work shares the ply's scheduling region (profiles/r02/fi/).
            while (p < plies && ((ply0 + (uint64_t)p) & 3) != 0) {
                const uint64_t g = ply0 + (uint64_t)p;
                ply(p, pick4(philox4(rng.seed, id, g >> 2, RNG_ACTION), (uint32_t)(g & 3)), nofill);
                ++p;
            }
            if (p + 4 <= plies) {
                U4 cur = philox4(rng.seed, id, (ply0 + (uint64_t)p) >> 2, RNG_ACTION);
                while (p + 4 <= plies) {
                    U4 nxt;  // (one unused block after the last group)
                    const uint64_t nb = ((ply0 + (uint64_t)p) >> 2) + 1;
                    ply(p, cur.x, [&]() __attribute__((always_inline)) {
                        nxt = philox4(rng.seed, id, nb, RNG_ACTION);
                        asm volatile("" : "+v"(nxt.x), "+v"(nxt.y), "+v"(nxt.z), "+v"(nxt.w));
                    });
                    ply(p + 1, cur.y, nofill);
                    ply(p + 2, cur.z, nofill);
                    ply(p + 3, cur.w, nofill);
                    cur = nxt;
                    p += 4;
                }
            }
            while (p < plies) {
                const uint64_t g = ply0 + (uint64_t)p;
                ply(p, pick4(philox4(rng.seed, id, g >> 2, RNG_ACTION), (uint32_t)(g & 3)), nofill);
                ++p;
            }
        };
        if (!slow) {
            // no opening bookkeeping when no board of the wave can have opening plies
            if (rng.init_rand == 0 && !__any((mt & 0xff00u) != 0)) fast(std::false_type{});
            else fast(std::true_type{});
            tally_from_signs(t0, t1, t2, cb, cd, cw);
            const bool tw = (mt & M_TURN_WHITE) != 0;
            s.white.w[0] = tw ? M : O;
            s.black.w[0] = tw ? O : M;
            s.legal.w[0] = L;
            s.meta = mt;
        } else {
            for (int p = 0; p < plies; ++p) {
                const uint64_t g = ply0 + (uint64_t)p;
                int a = -1, r = 0, d = 1, win = NO_DISK;
                if (!(s.meta & M_TERMINATED)) {
                    if (POLICY == OTH_POLICY_RANDOM || (s.meta >> M_RAND_SHIFT) > 0)
                        a = random_action<N>(s, action_draw(rng.seed, id, g));
                    else
                        a = policy_action<N, POLICY>(s, eng);
                    if ((s.meta >> M_RAND_SHIFT) > 0) s.meta -= 1u << M_RAND_SHIFT;
                    step_lane<N, Fills<N>, true>(s, a, flags, r, d, win, eng);
                    if (d) {
                        count_winner(win, cb, cd, cw);
                        reset_lane<N>(s, rng.seed, id, g, RNG_OPENING_AUTO, rng.init_rand);
                        eng.prime(s);
                    }
                }
                actions[(size_t)p * E + e] = a;
                rewards[(size_t)p * E + e] = r;
                dones[(size_t)p * E + e] = (uint8_t)d;
            }
        }
        store_lane<N>(s, boards, meta, legal, e);
    }
    tally(wdl, cb, cd, cw);
}

// play_rand_fast for multi-word boards (N >= 9, the FillsW engine): the same
// (mover, opponent) form with BB<W> words; every multi-word select is word by
// word (a selected member address puts the lane in scratch).
template <int N, bool OPEN = true, typename FILL = NoFill>
__device__ __forceinline__ void play_rand_fast_w(BB<Geo<N>::W>& M, BB<Geo<N>::W>& O, BB<Geo<N>::W>& L,
                                                 uint32_t& meta, const FillsW<N>& eng, uint32_t u, uint32_t flags,
                                                 const Rng& rng, uint32_t id, uint64_t g, int& a, int& r, int& d,
                                                 uint32_t& cb, uint32_t& cd, uint32_t& cw, const uint8_t* sel8,
                                                 const FILL& fill = FILL{}) {
    constexpr int W = Geo<N>::W;
    a = select_bit_tab(L, scale_index(u, popcount(L)), sel8);  // RandomPolicy (simple_policies.py:37-41); L != 0
    if constexpr (OPEN) meta -= (meta & 0xff00u) ? (1u << M_RAND_SHIFT) : 0u;
    const BB<W> m = square<W>(a);
    const BB<W> f = eng.flip(M, O, a);  // update_board (othello.py:391-410)
    const BB<W> Mn = M | f | m, On = O & ~f;
    const bool full = !any(~(Mn | On) & Geo<N>::BOARD);  // :425-426
    // a full board resets before the scan, as in play_rand_fast: the next mover's
    // scan runs on the start position, and only a double pass scans it again
    // (10x10: 1.692 -> 1.689 us per ply, profiles/r04/g/ab_term.jsonl)
    BB<W> nM, nO;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        nM.w[i] = full ? Start<N>::BLACK.w[i] : On.w[i];
        nO.w[i] = full ? Start<N>::WHITE.w[i] : Mn.w[i];
    }
    BB<W> Ln = eng.legal(nM, nO);  // the next mover's possible_moves (:436)
    fill();
    const bool pass = !any(Ln);  // never on the start position
    bool term = full;
    M = nM;
    O = nO;
    if (pass) {  // :437-440
        Ln = eng.legal(Mn, On);
        M = Mn;
        O = On;
        if (!any(Ln)) {  // nobody can move (:441-442): reset
            term = true;
            M = Start<N>::BLACK;
            O = Start<N>::WHITE;
            Ln = eng.legal(M, O);
        }
    }
    L = Ln;
    const uint32_t mover = meta;
    meta ^= pass ? 0u : M_TURN_WHITE;
    r = 0;
    d = term ? 1 : 0;
    if (term) {
        r = fast_terminal<N>(popcount(Mn), popcount(On), mover, flags, cb, cd, cw);
        meta = 0u;  // (without OPEN: no opening plies and none drawn, the scalar branch compiled out)
        if constexpr (OPEN) meta = reset_meta(rng.seed, id, g, RNG_OPENING_AUTO, rng.init_rand);
    }
}

// k_play_rand for multi-word boards (config 5's 10x10 and every N >= 9).
template <int N>
__global__ __launch_bounds__(BLOCK) void k_play_rand_w(uint64_t* __restrict__ boards, uint16_t* __restrict__ meta,
                                                       uint64_t* __restrict__ legal, int E, uint32_t flags, int plies,
                                                       int32_t* __restrict__ actions, int32_t* __restrict__ rewards,
                                                       uint8_t* __restrict__ dones,
                                                       unsigned long long* __restrict__ wdl, Rng rng, uint64_t ply0) {
    constexpr int W = Geo<N>::W;
    static_assert(W > 1, "multi-word boards");
    ply0 += *rng.ply_off;  // graph-region offset (oth_graph_end); 0 eagerly
    __shared__ __attribute__((aligned(16))) uint64_t lds_rays[FillsW<N>::RAY_WORDS];
    __shared__ __attribute__((aligned(16))) uint64_t lds_sel[256];
    for (int i = threadIdx.x; i < 256; i += BLOCK) lds_sel[i] = sel8_word((uint32_t)i);
    const uint8_t* sel8 = reinterpret_cast<const uint8_t*>(lds_sel);
    FillsW<N>::fill(lds_rays);  // (its barrier covers lds_sel)
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t cb = 0, cd = 0, cw = 0;
    if (e < E) {
        const uint32_t id = rng.id_base + (uint32_t)e;
        const FillsW<N> eng(0, lds_rays);
        Lane<N> s;
        load_lane<N>(s, boards, meta, legal, e);
        const bool tw0 = (s.meta & M_TURN_WHITE) != 0;
        BB<W> M, O, L = s.legal;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            M.w[i] = tw0 ? s.white.w[i] : s.black.w[i];
            O.w[i] = tw0 ? s.black.w[i] : s.white.w[i];
        }
        uint32_t mt = s.meta & (0xff00u | M_TURN_WHITE);
        eng.prime(s);
        const bool slow = __any((s.meta & M_TERMINATED) != 0 || !any(L));  // as k_play_rand
        int32_t* act_p = actions + e;
        int32_t* rew_p = rewards + e;
        uint8_t* done_p = dones + e;
        uint32_t t0 = 0, t1 = 0, t2 = 0;  // play_rand_fast_w's tally (tally_from_signs)
        // OPEN: some board of the wave may have or draw random-opening plies; without,
        // the opening bookkeeping and the reset's opening draw are compiled out
        auto fast = [&](auto OPENC) __attribute__((always_inline)) {
            constexpr bool OPEN = decltype(OPENC)::value;
            auto ply = [&](uint64_t g, uint32_t u, const auto& fill) __attribute__((always_inline)) {
                int a, r, d;
                play_rand_fast_w<N, OPEN>(M, O, L, mt, eng, u, flags, rng, id, g, a, r, d, t0, t1, t2, sel8, fill);
                *act_p = a;
                *rew_p = r;
                *done_p = (uint8_t)d;
                act_p += E;
                rew_p += E;
                done_p += E;
            };
            // Philox block g/4 serves plies 4k..4k+3 (g uniform: scalar branches).
            // Two-word boards compute the next block in the current group's first ply
            // (as k_play_rand: 10x10 +5 %); boards of 3+ words, already past 256 VGPRs,
            // at each group's start (the pipelined form: 12x12 -4 %)
            const NoFill nofill;
            int p = 0;
            if constexpr (W > 2) {
                while (p < plies) {
                    const uint64_t g = ply0 + (uint64_t)p;
                    const U4 d4 = philox4(rng.seed, id, g >> 2, RNG_ACTION);
                    if ((g & 3) == 0 && p + 4 <= plies) {
                        ply(g, d4.x, nofill);
                        ply(g + 1, d4.y, nofill);
                        ply(g + 2, d4.z, nofill);
                        ply(g + 3, d4.w, nofill);
                        p += 4;
                    } else {
                        ply(g, pick4(d4, (uint32_t)(g & 3)), nofill);
                        ++p;
                    }
                }
            } else {
                while (p < plies && ((ply0 + (uint64_t)p) & 3) != 0) {
                    const uint64_t g = ply0 + (uint64_t)p;
                    ply(g, pick4(philox4(rng.seed, id, g >> 2, RNG_ACTION), (uint32_t)(g & 3)), nofill);
                    ++p;
                }
                if (p + 4 <= plies) {
                    U4 cur = philox4(rng.seed, id, (ply0 + (uint64_t)p) >> 2, RNG_ACTION);
                    while (p + 4 <= plies) {
                        const uint64_t g = ply0 + (uint64_t)p;
                        U4 nxt;  // (one unused block after the last group)
                        ply(g, cur.x, [&]() __attribute__((always_inline)) {
                            nxt = philox4(rng.seed, id, (g >> 2) + 1, RNG_ACTION);
                            asm volatile("" : "+v"(nxt.x), "+v"(nxt.y), "+v"(nxt.z), "+v"(nxt.w));
                        });
                        ply(g + 1, cur.y, nofill);
                        ply(g + 2, cur.z, nofill);
                        ply(g + 3, cur.w, nofill);
                        cur = nxt;
                        p += 4;
                    }
                }
                while (p < plies) {
                    const uint64_t g = ply0 + (uint64_t)p;
                    ply(g, pick4(philox4(rng.seed, id, g >> 2, RNG_ACTION), (uint32_t)(g & 3)), nofill);
                    ++p;
                }
            }
        };
        if (!slow) {
            // (one loop for both: 10x10 without openings 1.422 -> 1.447 us per ply, profiles/r06/n)
            if (rng.init_rand == 0 && !__any((mt & 0xff00u) != 0)) fast(std::false_type{});
            else fast(std::true_type{});
            tally_from_signs(t0, t1, t2, cb, cd, cw);
            const bool tw = (mt & M_TURN_WHITE) != 0;
#pragma unroll
            for (int i = 0; i < W; ++i) {
                s.white.w[i] = tw ? M.w[i] : O.w[i];
                s.black.w[i] = tw ? O.w[i] : M.w[i];
            }
            s.legal = L;
            s.meta = mt;
        } else {
            for (int p = 0; p < plies; ++p) {
                const uint64_t g = ply0 + (uint64_t)p;
                int a = -1, r = 0, d = 1, win = NO_DISK;
                if (!(s.meta & M_TERMINATED)) {
                    a = random_action<N>(s, action_draw(rng.seed, id, g));
                    if ((s.meta >> M_RAND_SHIFT) > 0) s.meta -= 1u << M_RAND_SHIFT;
                    step_lane<N, FillsW<N>, true>(s, a, flags, r, d, win, eng);
                    if (d) {
                        count_winner(win, cb, cd, cw);
                        reset_lane<N>(s, rng.seed, id, g, RNG_OPENING_AUTO, rng.init_rand);
                        eng.prime(s);
                    }
                }
                act_p[(size_t)p * E] = a;
                rew_p[(size_t)p * E] = r;
                done_p[(size_t)p * E] = (uint8_t)d;
            }
        }
        store_lane<N>(s, boards, meta, legal, e);
    }
    tally(wdl, cb, cd, cw);
}

}  // namespace oth_dev
