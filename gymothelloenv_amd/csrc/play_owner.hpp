// play_owner.hpp -- a board's owner in the kernels that play a chosen move: k_play_search (play_search.hpp: the
// move is the search's) and k_play_net (play_net.hpp: the move is the network's).  Both cut a board's control
// flow where it may need a chosen move: the owner lane holds its board's Lane<N> in registers for the whole
// call, `advance` takes the board through everything that needs no chosen move (the protagonist's ply,
// random-opening plies, a terminated board's plies, tallies, auto-reset: a per-board phase that only moves
// forward) until it wants a move or is finished for this call, `apply` plays the chosen move, `finish` stores
// the board, the call's outputs and the tallies.  One text for both kernels: oth_step_policy's contract in play
// mode, oth_reset_vs's / oth_step_vs's in the vs modes.
#pragma once
#include "vs.hpp"

namespace oth_dev {

constexpr int PS_PLAY = 0, PS_STEP_VS = 1, PS_RESET_VS = 2;
constexpr int PS_RUNTIME = -1;  // PlayOwner's MODE: the mode is a (block-uniform) kernel argument
// a board's phase in the vs modes (vs.hpp's control flow cut where it may need a chosen move), in the order it is gone through
constexpr int VS_PRE = 0,     // the opponent replies before the protagonist's ply
    VS_PROT = 1,              // the protagonist's ply
    VS_POST = 2,              // the opponent replies after it
    VS_END = 3,               // plies, tallies, auto-reset
    VS_RESET_REPLY = 4,       // the opponent's replies of a reset (no openings, nothing reported)
    VS_DONE = 5;

// MODE PS_PLAY: ctr the first ply's counter; the vs modes: ctr the call's counter.
// Outputs: actions / rewards / dones / fb_ply [n_plies][E] in play mode; rewards / dones / plies_out / fb_cnt [E]
// in PS_STEP_VS; none in PS_RESET_VS (mask: the boards to reset, NULL for all).  Each may be NULL.
template <int N, int MODE>
struct PlayOwner {
    static constexpr int W = Geo<N>::W;
    // the call
    int mode_rt, E, n_plies;
    uint32_t flags;
    const int32_t* act_in;
    int32_t *actions, *rewards;
    uint8_t *dones, *fb_ply;
    Rng rng;
    uint64_t ctr;
    // the board
    Lane<N> s;
    bool owner, protw;
    int e;
    uint32_t id;
    uint64_t gbase;
    int p;                               // play: the board's next ply
    int ph, r, d, win, plies, nfb;       // vs: phase and the call's results
    uint32_t j;                          // vs: the call's next draw
    uint32_t cb, cd, cw, vw, vd, vl;

    __device__ __forceinline__ int mode() const { return MODE == PS_RUNTIME ? mode_rt : MODE; }

    // lane `slot` of a block that owns the boards e0 .. e0 + ne - 1 (an owner when slot < ne); ctr with the
    // graph-region offset added
    __device__ __forceinline__ void init(int mode_, int slot, long long e0, int ne, uint64_t* __restrict__ boards,
                                         uint16_t* __restrict__ meta, uint64_t* __restrict__ legal, int E_,
                                         uint32_t flags_, int n_plies_, const int32_t* __restrict__ act_in_,
                                         const int8_t* __restrict__ prot, const uint8_t* __restrict__ mask,
                                         int32_t* __restrict__ actions_, int32_t* __restrict__ rewards_,
                                         uint8_t* __restrict__ dones_, uint8_t* __restrict__ fb_ply_, const Rng& rng_,
                                         uint64_t ctr_) {
        mode_rt = mode_;
        E = E_;
        n_plies = n_plies_;
        flags = flags_;
        act_in = act_in_;
        actions = actions_;
        rewards = rewards_;
        dones = dones_;
        fb_ply = fb_ply_;
        rng = rng_;
        ctr = ctr_;
        owner = slot < ne;
        e = (int)(e0 + (owner ? slot : 0));
        if (mode() == PS_RESET_VS && owner && mask && !mask[e]) owner = false;
        id = rng.id_base + (uint32_t)e;
        gbase = ctr * VS_PLIES_PER_CALL;
        s.black = zero<W>();
        s.white = zero<W>();
        s.legal = zero<W>();
        s.meta = M_TERMINATED;
        protw = true;
        p = 0;
        ph = VS_DONE, r = 0, d = 1, win = NO_DISK, plies = 0, nfb = 0;
        j = 0;
        cb = cd = cw = vw = vd = vl = 0;
        if (owner) {
            if (mode() != PS_PLAY) protw = prot ? prot[e] == WHITE_DISK : true;
            if (mode() == PS_RESET_VS) {
                reset_lane<N>(s, rng.seed, id, ctr, RNG_OPENING_RESET, rng.init_rand);
                ph = VS_RESET_REPLY;
            } else {
                load_lane<N>(s, boards, meta, legal, e);
                if (mode() == PS_STEP_VS && !(s.meta & M_TERMINATED)) {
                    d = 0;
                    ph = VS_PRE;
                }
            }
        }
    }
    __device__ __forceinline__ bool has_move() const { return any(s.legal & Geo<N>::BOARD); }
    // the global index of the ply the board is at: the index action_draw would use for a random move of it
    __device__ __forceinline__ uint64_t ply_index() const {
        return mode() == PS_PLAY ? ctr + (uint64_t)p : gbase + (uint64_t)j;
    }
    // play: ply p's outputs
    __device__ __forceinline__ void record(int a, int rr, int dd, int fb) {
        const size_t o = (size_t)p * (size_t)E + (size_t)e;
        if (actions) actions[o] = a;
        if (rewards) rewards[o] = rr;
        if (dones) dones[o] = (uint8_t)dd;
        if (fb_ply) fb_ply[o] = (uint8_t)fb;
    }
    // play: ply p of a live board (k_play's ply)
    __device__ __forceinline__ void play_ply(int a, int fb) {
        const Solo<N> eng(0, nullptr);
        int rr, dd, ww;
        step_lane<N>(s, a, flags, rr, dd, ww, eng);
        if (dd) {
            count_winner(ww, cb, cd, cw);
            if (flags & OTH_AUTO_RESET) reset_lane<N>(s, rng.seed, id, ctr + (uint64_t)p, RNG_OPENING_AUTO, rng.init_rand);
        }
        record(a, rr, dd, fb);
        ++p;
    }
    // vs: one ply; a reset's replies report nothing (reset_vs_lane)
    __device__ __forceinline__ void vs_ply(int a) {
        const Solo<N> eng(0, nullptr);
        if (ph == VS_RESET_REPLY) {
            int rr, dd, ww;
            step_lane<N>(s, a, flags, rr, dd, ww, eng);
        } else {
            step_lane<N>(s, a, flags, r, d, win, eng);
        }
    }
    // the board through everything that needs no chosen move; true: it wants one now
    __device__ __forceinline__ bool advance() {
        if (mode() == PS_PLAY) {
            while (p < n_plies) {
                if (s.meta & M_TERMINATED) {
                    record(-1, 0, 1, 0);
                    ++p;
                    continue;
                }
                if ((s.meta >> M_RAND_SHIFT) > 0) {  // a random-opening ply
                    const int a = random_action<N>(s, action_draw(rng.seed, id, ctr + (uint64_t)p));
                    s.meta -= 1u << M_RAND_SHIFT;
                    play_ply(a, 0);
                    continue;
                }
                if (!has_move()) {  // GreedyPolicy's None: the invalid path
                    play_ply(-1, 0);
                    continue;
                }
                return true;
            }
            return false;
        } else {
            const Solo<N> eng(0, nullptr);
            for (;;) {
                if (ph == VS_DONE) return false;
                if (ph == VS_PROT) {
                    int a = act_in[e];
                    const uint64_t g = gbase + j++;
                    if ((s.meta >> M_RAND_SHIFT) > 0) {  // opening ply: the protagonist's action is replaced too
                        a = random_action<N>(s, action_draw(rng.seed, id, g));
                        s.meta -= 1u << M_RAND_SHIFT;
                    }
                    step_lane<N>(s, a, flags, r, d, win, eng);
                    ph = d ? VS_END : VS_POST;
                    continue;
                }
                if (ph == VS_END) {
                    plies = (int)j;
                    ph = VS_DONE;
                    if (d) {
                        count_winner(win, cb, cd, cw);
                        const int pcol = protw ? WHITE_DISK : BLACK_DISK;
                        vw += win == pcol;
                        vd += win == NO_DISK;
                        vl += win == -pcol;
                        if (flags & OTH_AUTO_RESET) {
                            reset_lane<N>(s, rng.seed, id, ctr, RNG_OPENING_AUTO, rng.init_rand);
                            ph = VS_RESET_REPLY;
                        }
                    }
                    continue;
                }
                // the reply phases: the opponent moves while it is to move and the game is on
                const bool term = (s.meta & M_TERMINATED) != 0;
                if (term || ((s.meta & M_TURN_WHITE) != 0) == protw) {
                    if (ph == VS_PRE && !term) {
                        ph = VS_PROT;
                    } else if (ph == VS_RESET_REPLY) {
                        ph = VS_DONE;
                    } else {  // the game ended before the protagonist's ply, or the replies after it are over
                        r = -r;
                        ph = VS_END;
                    }
                    continue;
                }
                if (ph != VS_RESET_REPLY && (s.meta >> M_RAND_SHIFT) > 0) {
                    const int a = random_action<N>(s, action_draw(rng.seed, id, gbase + j++));
                    s.meta -= 1u << M_RAND_SHIFT;
                    vs_ply(a);
                    continue;
                }
                if (!has_move()) {
                    ++j;
                    vs_ply(-1);
                    continue;
                }
                return true;
            }
        }
    }
    // the chosen move of a board that wanted one (fb: it was a fallback's)
    __device__ __forceinline__ void apply(int a, int fb) {
        if (mode() == PS_PLAY) {
            play_ply(a, fb);
        } else {
            ++j;
            nfb += fb;
            vs_ply(a);
        }
    }
    // the board back, the call's outputs, the tallies into the handle's W/D/L slot `slot` (atomics without a
    // return value: blocks may share a slot).  Every lane of the wave calls this.
    __device__ __forceinline__ void finish(uint64_t* __restrict__ boards, uint16_t* __restrict__ meta,
                                           uint64_t* __restrict__ legal, int32_t* __restrict__ plies_out,
                                           int32_t* __restrict__ fb_cnt, unsigned long long* __restrict__ wdl,
                                           unsigned long long* __restrict__ wdl_vs, size_t slot) {
        if (owner) {
            store_lane<N>(s, boards, meta, legal, e);
            if (mode() == PS_STEP_VS) {
                if (rewards) rewards[e] = r;
                if (dones) dones[e] = (uint8_t)d;
                if (plies_out) plies_out[e] = plies;
                if (fb_cnt) fb_cnt[e] = nfb;
            }
        }
        if (mode() != PS_RESET_VS) {
            const int lane = threadIdx.x & 63;
            cb = wave_sum(cb);
            cd = wave_sum(cd);
            cw = wave_sum(cw);
            if (lane == 0 && wdl) {
                if (cb) atomicAdd(wdl + 4 * slot + 0, (unsigned long long)cb);
                if (cd) atomicAdd(wdl + 4 * slot + 1, (unsigned long long)cd);
                if (cw) atomicAdd(wdl + 4 * slot + 2, (unsigned long long)cw);
            }
            if (mode() == PS_STEP_VS) {
                vw = wave_sum(vw);
                vd = wave_sum(vd);
                vl = wave_sum(vl);
                if (lane == 0 && wdl_vs) {
                    if (vw) atomicAdd(wdl_vs + 4 * slot + 0, (unsigned long long)vw);
                    if (vd) atomicAdd(wdl_vs + 4 * slot + 1, (unsigned long long)vd);
                    if (vl) atomicAdd(wdl_vs + 4 * slot + 2, (unsigned long long)vl);
                }
            }
        }
    }
};

}  // namespace oth_dev
