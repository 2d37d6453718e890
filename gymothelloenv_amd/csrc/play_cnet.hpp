// play_cnet.hpp -- the convolutional network as a player: oth_play_cnet, oth_reset_vs_cnet, oth_step_vs_cnet
// (oth_play_net and its vs calls with the move chosen by oth_cnet_eval's computation).  The spec is the header's
// comment on oth_play_cnet: P(board, p) of play_net.hpp with z and prior[] the conv net's.
//
// The move's shared core (the argmax key, the draw's target, the cumulative scan, a row's move on the host) is
// play_net.hpp's, the network's pieces (cnet_conv, cnet_head, the wave reductions) are cnet_dev.hpp's: this file
// holds only the rounds that join the two.
//
// Device mapping (k_play_cnet): a workgroup of four waves owns RB = cnet_rows_per_block(ST) consecutive boards
// for the whole call (4 at N = 4, 2 at N = 5, 1 from N = 6) and keeps k_cnet_eval's LDS images of them, in rounds:
//   * the lanes < RB of wave 0 own the boards (play_owner.hpp): an owner advances its board until it wants the
//     network's move or is finished for this call, and publishes (mover, opponent, stored moves, which side's
//     network, whether the move is drawn) to LDS;
//   * after a barrier every thread reads the want flags -- the loop's exit test is workgroup-uniform -- and the
//     workgroup leaves when no row wants a move;
//   * a pass: all threads expand the published words into the three byte planes (the whole interior, 0 and 1
//     alike, zeros for a row that does not take this pass; the halo was zeroed once), then stem, blocks and head
//     run with k_cnet_eval's barriers, the loop bounds and shifts taken from the pass's own side.  One pass when
//     both sides are one network or every wanting row wants the same side, else one a side.  Every lane executes
//     every MFMA;
//   * the move, a wave a row: the argmax key over the row's logits on M by a wave max; for a drawing row the
//     integer softmax (the maximum is the key's, the sum a wave sum), the priors written over the logits, and
//     after a barrier the owner's scan over them;
//   * the owners apply the moves through step_lane.
// Every round places a disc on every wanting board; the rounds are bounded as k_play_net's are.
#pragma once
#include "cnet.hpp"
#include "play_net.hpp"

#if defined(__HIPCC__)
#include "cnet_dev.hpp"

namespace oth_dev {

// one colour's oth_cnet_policy as the kernel takes it
struct PlayCnetSide {
    CnetGeo geo;
    const uint8_t* blob;
    int sample_discs;
};
// both colours': one kernel argument, so that a pass picks its side by an index into the argument segment
struct PlayCnetSides {
    PlayCnetSide s[2];  // black's, white's
};

// the published rows behind k_cnet_eval's images: mover, opponent and stored moves (RB x W words each), then a
// key word a row, then 64 bytes for the want and draw flags (four of each)
__host__ __device__ inline size_t play_cnet_lds_bytes(const CnetGeo& geo, int RB) {
    return cnet_lds_bytes(geo, RB) + (size_t)RB * (3u * (size_t)geo.W + 1u) * 8u + 64u;
}

// all 32 head bytes of a blob: both tags and the 16 shift bytes (k_cnet_eval's test)
__device__ __forceinline__ bool play_cnet_head_ok(const CnetGeo& geo, const uint8_t* __restrict__ blob) {
    const uint64_t* hd = reinterpret_cast<const uint64_t*>(blob);
    uint64_t s0 = 0, s1 = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        s0 |= (uint64_t)geo.shifts[i] << (8 * i);
        s1 |= (uint64_t)geo.shifts[8 + i] << (8 * i);
    }
    return hd[0] == geo.tag0() && hd[1] == geo.tag1() && hd[2] == s0 && hd[3] == s1;
}

__device__ __forceinline__ uint64_t play_cnet_wave_max(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, d);
        v = o > v ? o : v;
    }
    return v;
}

// mode, the sides, same, the outputs and ctr: as k_play_net takes them.  The two sides have C channels each; blocks,
// shifts and weights may differ.  A blob of another geometry or other shifts: nothing is changed.
template <int N, int C>
__global__ __launch_bounds__(CNET_THREADS) void k_play_cnet(
    uint64_t* __restrict__ boards, uint16_t* __restrict__ meta, uint64_t* __restrict__ legal, int E, uint32_t flags,
    int mode, PlayCnetSides sides, int same, int n_plies, const int32_t* __restrict__ act_in,
    const int8_t* __restrict__ prot, const uint8_t* __restrict__ mask, int32_t* __restrict__ actions,
    int32_t* __restrict__ rewards, uint8_t* __restrict__ dones, int32_t* __restrict__ plies_out,
    unsigned long long* __restrict__ wdl, unsigned long long* __restrict__ wdl_vs, Rng rng, uint64_t ctr) {
    constexpr int W = Geo<N>::W, NN = N * N, ST = (NN + 15) / 16, RB = ST >= 3 ? 1 : (ST == 2 ? 2 : 4);
    constexpr int NP = N + 2, P2 = NP * NP;
    static_assert(NN <= 256 && RB <= 4, "a square fits the key's low byte; a row a wave");
    extern __shared__ uint4 lds[];
    const PlayCnetSide &side_b = sides.s[0], &side_w = sides.s[1];
    // the heads first, workgroup-uniformly: a blob packed for something else changes nothing
    if (!play_cnet_head_ok(side_b.geo, side_b.blob)) return;
    if (!same && !play_cnet_head_ok(side_w.geo, side_w.blob)) return;
    ctr += *rng.ply_off;  // graph-region offset (oth_graph_end); 0 eagerly
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long e0 = (long long)blockIdx.x * RB;
    const int ne = (int)(E - e0 < RB ? E - e0 : RB);

    // ---- the LDS: k_cnet_eval's images (one layout for both sides: n and C are theirs in common), then the
    // published rows
    const CnetGeo& g0 = side_b.geo;
    const size_t image = (size_t)RB * P2 * C;
    uint8_t* h = reinterpret_cast<uint8_t*>(lds);
    uint8_t* t = h + image;
    uint8_t* pl = t + image;
    int32_t* zs = reinterpret_cast<int32_t*>(pl + (((size_t)RB * 3u * P2 + 15u) & ~(size_t)15u));
    int32_t* vsum = zs + (((size_t)RB * NN + 3u) & ~(size_t)3u);
    uint64_t* g_M = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(lds) + cnet_lds_bytes(g0, RB));
    uint64_t* g_O = g_M + RB * W;
    uint64_t* g_L = g_O + RB * W;
    uint64_t* g_key = g_L + RB * W;                           // a row's argmax key
    int32_t* g_want = reinterpret_cast<int32_t*>(g_key + RB);  // 0: no move wanted this round; 1: black's network's; 2: white's
    int32_t* g_draw = g_want + 4;                             // the row's move is drawn from the priors
    const int words = (int)(play_cnet_lds_bytes(g0, RB) / 16u);
    for (int i = tid; i < words; i += CNET_THREADS) lds[i] = make_uint4(0u, 0u, 0u, 0u);

    // ---- the owners' state and control flow (play_owner.hpp)
    PlayOwner<N, PS_RUNTIME> o;
    o.init(mode, tid, e0, ne, boards, meta, legal, E, flags, n_plies, act_in, prot, mask, actions, rewards, dones,
           nullptr, rng, ctr);
    __syncthreads();

    // ---- the rounds
    const int QT = RB * ST;
    for (;;) {
        bool want = false, draw = false;
        if (tid < RB) {
            if (o.owner) want = o.advance();
            int side = 0;
            if (want) {
                const bool tw = (o.s.meta & M_TURN_WHITE) != 0;
                const BB<W> M = pick(tw, o.s.white, o.s.black), O = pick(tw, o.s.black, o.s.white);
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    g_M[tid * W + k] = M.w[k];
                    g_O[tid * W + k] = O.w[k];
                    g_L[tid * W + k] = o.s.legal.w[k];
                }
                side = mode == PS_PLAY && tw ? 2 : 1;
                draw = popcount(o.s.black | o.s.white) < (side == 2 ? side_w.sample_discs : side_b.sample_discs);
            }
            g_want[tid] = side;
            g_draw[tid] = draw ? 1 : 0;
        }
        __syncthreads();
        // which rows want which network, read from LDS after the barrier: the tests below are workgroup-uniform
        bool want_b = false, want_w = false;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            want_b |= g_want[rb] == 1;
            want_w |= g_want[rb] == 2;
        }
        if (!want_b && !want_w) break;
        int a_sel = -1;
        for (int k = 1; k <= 2; ++k) {
            // one network: a single pass over every wanting row; two: a pass a side that is wanted
            if (same ? k == 2 : !(k == 1 ? want_b : want_w)) continue;
            const PlayCnetSide& sd = sides.s[k - 1];
            const CnetGeo& geo = sd.geo;
            // the three planes of every row as bytes of 0 or 1 inside the halo: the whole interior, every pass
            for (int i = tid; i < RB * 3 * NN; i += CNET_THREADS) {
                const int rb = i / (3 * NN), rest = i - rb * 3 * NN;
                const int p = rest / NN, a = rest - p * NN;
                const bool mine = same ? g_want[rb] != 0 : g_want[rb] == k;
                const uint64_t* src = (p == 0 ? g_M : (p == 1 ? g_O : g_L)) + rb * W;
                const int y = a / N;
                pl[(rb * 3 + p) * P2 + (y + 1) * NP + (a - y * N) + 1] =
                    mine ? (uint8_t)((src[a >> 6] >> (a & 63)) & 1u) : (uint8_t)0;
            }
            if (tid < RB) vsum[tid] = 0;  // cnet_head adds into it
            __syncthreads();
            cnet_conv<C, CNET_STEM>(geo, sd.blob + geo.off_stem(), geo.shift_stem, nullptr, h, pl, QT, wave, lane);
            __syncthreads();
            for (int b = 0; b < geo.B; ++b) {
                cnet_conv<C, CNET_FIRST>(geo, sd.blob + geo.off_conv(2 * b), geo.shifts[2 * b], h, t, pl, QT, wave, lane);
                __syncthreads();
                cnet_conv<C, CNET_SECOND>(geo, sd.blob + geo.off_conv(2 * b + 1), geo.shifts[2 * b + 1], t, h, pl, QT,
                                          wave, lane);
                __syncthreads();
            }
            cnet_head<C>(geo, sd.blob, h, zs, vsum, QT, wave, lane);
            __syncthreads();
            // a row a wave: the argmax key; for a drawing row the integer softmax, the priors over the logits
            if (wave < RB) {
                const int rb = wave;
                if (same ? g_want[rb] != 0 : g_want[rb] == k) {
                    int32_t z[W];
                    bool in_m[W];
                    uint64_t key = 0;
#pragma unroll
                    for (int i = 0; i < W; ++i) {
                        const int a = lane + 64 * i;
                        z[i] = a < NN ? zs[rb * NN + a] : 0;
                        in_m[i] = a < NN && ((g_L[rb * W + i] >> lane) & 1u);
                        if (in_m[i]) {
                            const uint64_t kk = net_move_key(z[i], a);
                            key = kk > key ? kk : key;
                        }
                    }
                    key = play_cnet_wave_max(key);
                    if (lane == 0) g_key[rb] = key;
                    if (g_draw[rb] && key) {
                        const int32_t m = (int32_t)((int64_t)(key >> 8) - 2147483648ll);  // the largest logit on M
                        uint32_t e[W];
                        uint64_t S = 0;
#pragma unroll
                        for (int i = 0; i < W; ++i) {
                            e[i] = in_m[i] ? net_exp(m, z[i], geo.policy_shift) : 0u;
                            S += e[i];
                        }
                        S = cnet_wave_sum(S);
#pragma unroll
                        for (int i = 0; i < W; ++i) {
                            const int a = lane + 64 * i;
                            if (a < NN) zs[rb * NN + a] = in_m[i] ? net_prior(e[i], S) : 0;
                        }
                    }
                }
            }
            __syncthreads();  // the rows' keys and priors, written by their waves, are read by their owners
            if (want && (same || g_want[tid] == k)) {
                if (draw) {
                    const auto pr = [&](int a) { return zs[tid * NN + a]; };
                    const uint32_t u = net_move_word(rng.seed, o.id, o.ply_index());
                    a_sel = net_sample_square(NN, g_L + tid * W, pr, net_draw_target(u, net_prior_sum(NN, g_L + tid * W, pr)));
                } else {
                    a_sel = net_key_square(g_key[tid]);
                }
            }
            __syncthreads();  // zs and the planes are free again
        }
        if (want) o.apply(a_sel, 0);
    }

    // ---- the boards back, the call's outputs, the tallies: the handle has a W/D/L slot per 16 boards; the
    // workgroups of one 16 share theirs (atomics).  The owners are wave 0's.
    if (wave == 0) o.finish(boards, meta, legal, plies_out, nullptr, wdl, wdl_vs, (size_t)(e0 / 16));
}

}  // namespace oth_dev
#endif
