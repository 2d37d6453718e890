// play_net.hpp -- the network as a player: oth_play_net (oth_step_policy with the mover's move chosen by
// oth_net_eval's computation, a network per colour) and oth_reset_vs_net / oth_step_vs_net (oth_reset_vs /
// oth_step_vs with the embedded opponent's move chosen so).  The spec is the header's comment on oth_play_net.
//
// The network's move P(board, p): with M the stored possible_moves on the board's squares, z and prior[] what
// oth_net_eval gives for the row and D the discs on the board, the move is the square of M with the largest z
// (the lowest of equals) when D >= p.sample_discs, else a draw in proportion to the priors: the first square
// in ascending order whose cumulative prior exceeds floor(u P / 2^32), P the priors' sum over M, u word 0 of
// the Philox block (id, g lo, g hi, purpose 7).
//
// The shared core (the part outside __HIPCC__: the argmax key, the draw's target, the cumulative scan and one
// row's move on the host) is plain host / device code: tests/host/play_net_host.cpp compiles the same text
// with g++.
//
// Device mapping (k_play_net): a block of one wave over 16 boards, in rounds:
//   * the lanes < 16 own their boards (play_owner.hpp, the text k_play_search's owners run): in a round every
//     owner advances its board until it wants the network's move or is finished for this call, and publishes
//     (mover, opponent, stored moves, which side's network) to LDS;
//   * after a barrier the wave reads which rows want which network -- the loop's exit test is block-uniform --
//     and leaves when none does;
//   * otherwise the wave evaluates the tile of 16 rows (net_dev.hpp's net_eval_tile: lane 16 g + c carries row
//     c) with the wanted network: once when every wanting row wants the same one, else once a side, a row
//     taking its side's result.  Rows that want nothing are evaluated as rows of zeros and ignored: every lane
//     executes every MFMA;
//   * the argmax key is the max over the row's four lanes (two shuffles); a sampling row's owner scans the
//     row's priors in the LDS; the owners apply the move through step_lane.
// Every round places a disc on every wanting board, and the rounds are bounded by n_plies (play) or the
// board's phase sequence (vs), exactly as k_play_search's.
#pragma once
#include "net.hpp"

namespace oth {

constexpr int NET_SAMPLE_DISCS_MAX = 257;   // sample_discs in [0, 257]: above every board's disc count
constexpr uint32_t NET_MOVE_PURPOSE = 7u;   // the draw's Philox purpose (state.hpp RNG_NET_MOVE)

// the max of (z + 2^31) << 8 | (255 - square) is the lowest square of the largest logit; 0: no square yet
OTH_HD uint64_t net_move_key(int32_t z, int a) {
    return (uint64_t)((int64_t)z + 2147483648ll) << 8 | (uint64_t)(255 - a);
}
OTH_HD int net_key_square(uint64_t key) { return 255 - (int)(key & 255u); }
// r = floor(u P / 2^32)
OTH_HD uint32_t net_draw_target(uint32_t u, uint32_t P) { return (uint32_t)(((uint64_t)u * (uint64_t)P) >> 32); }
OTH_HD uint32_t net_move_word(uint64_t seed, uint32_t id, uint64_t g) { return philox_x(seed, id, g, NET_MOVE_PURPOSE); }
// the first square of M (words, squares < nn) in ascending order whose cumulative prior exceeds r; -1: none
template <class Prior>
OTH_HD int net_sample_square(int nn, const uint64_t* M, Prior prior, uint32_t r) {
    uint64_t c = 0;
    for (int a = 0; a < nn; ++a) {
        if (!((M[a >> 6] >> (a & 63)) & 1u)) continue;
        c += (uint64_t)(uint32_t)prior(a);
        if (c > (uint64_t)r) return a;
    }
    return -1;
}
// the priors' sum over M
template <class Prior>
OTH_HD uint32_t net_prior_sum(int nn, const uint64_t* M, Prior prior) {
    uint32_t P = 0;
    for (int a = 0; a < nn; ++a)
        if ((M[a >> 6] >> (a & 63)) & 1u) P += (uint32_t)prior(a);
    return P;
}

// P of one row on the host (the tests' host build): z int32[nn (+ 1)], prior int32[nn], stored the row's legal
// words, discs D, u the draw's word.  -1 for a row whose stored mask is empty on the board.
inline int net_move_row(int nn, const int32_t* z, const int32_t* prior, const uint64_t* stored, int discs,
                        int sample_discs, uint32_t u) {
    uint64_t key = 0;
    for (int a = 0; a < nn; ++a)
        if ((stored[a >> 6] >> (a & 63)) & 1u) {
            const uint64_t k = net_move_key(z[a], a);
            key = k > key ? k : key;
        }
    if (!key) return -1;
    if (discs >= sample_discs) return net_key_square(key);
    const auto pr = [&](int a) { return prior[a]; };
    return net_sample_square(nn, stored, pr, net_draw_target(u, net_prior_sum(nn, stored, pr)));
}

}  // namespace oth

#if defined(__HIPCC__)
#include "net_dev.hpp"
#include "play_owner.hpp"

namespace oth_dev {

static_assert(RNG_NET_MOVE == NET_MOVE_PURPOSE, "one purpose word");

constexpr int PLAY_NET_GROUP = NET_ROWS;  // boards a block: a tile of rows

// one colour's oth_net_policy as the kernel takes it
struct PlayNetSide {
    NetGeo geo;
    const uint8_t* blob;
    int sample_discs;
};

// mode (block-uniform, PS_*) PS_PLAY: side_b is black's network, side_w white's, ctr the first ply's counter; the
// vs modes: both are the opponent's, ctr the call's counter.  same: both sides are one network (one evaluation a
// round).  Outputs: actions / rewards / dones [n_plies][E] in play mode; rewards / dones / plies_out [E] in
// PS_STEP_VS; none in PS_RESET_VS (mask: the boards to reset, NULL for all).  Each may be NULL.  A blob of
// another geometry or other shifts: nothing is changed.
template <int N, int KS>
__global__ __launch_bounds__(64) void k_play_net(
    uint64_t* __restrict__ boards, uint16_t* __restrict__ meta, uint64_t* __restrict__ legal, int E, uint32_t flags,
    int mode, PlayNetSide side_b, PlayNetSide side_w, int same, int n_plies, const int32_t* __restrict__ act_in,
    const int8_t* __restrict__ prot, const uint8_t* __restrict__ mask, int32_t* __restrict__ actions,
    int32_t* __restrict__ rewards, uint8_t* __restrict__ dones, int32_t* __restrict__ plies_out,
    unsigned long long* __restrict__ wdl, unsigned long long* __restrict__ wdl_vs, Rng rng, uint64_t ctr) {
    constexpr int W = Geo<N>::W, NN = N * N, G = PLAY_NET_GROUP, OT = (NN + 1 + 15) / 16;
    static_assert(NN <= 256, "a square fits the key's low byte");
    __shared__ int32_t zs[OT * 4 * 64];                       // net_eval_tile's: the rows' priors after it
    __shared__ uint64_t g_M[G][W], g_O[G][W], g_L[G][W];      // a wanting board's mover, opponent and stored moves
    __shared__ int g_want[G];                                 // 0: no move wanted this round; 1: black's network's; 2: white's
    // the tags first, block-uniformly: a blob packed for something else changes nothing
    {
        const uint64_t* tb = reinterpret_cast<const uint64_t*>(side_b.blob);
        if (tb[0] != side_b.geo.tag0() || tb[1] != side_b.geo.tag1()) return;
        const uint64_t* tw = reinterpret_cast<const uint64_t*>(side_w.blob);
        if (!same && (tw[0] != side_w.geo.tag0() || tw[1] != side_w.geo.tag1())) return;
    }
    ctr += *rng.ply_off;  // graph-region offset (oth_graph_end); 0 eagerly
    const int lane = threadIdx.x, c = lane & 15;
    const long long e0 = (long long)blockIdx.x * G;
    const int ne = (int)(E - e0 < G ? E - e0 : G);

    // ---- the owners' state and control flow (play_owner.hpp)
    PlayOwner<N, PS_RUNTIME> o;
    o.init(mode, lane, e0, ne, boards, meta, legal, E, flags, n_plies, act_in, prot, mask, actions, rewards, dones,
           nullptr, rng, ctr);
    if (lane < G) {
#pragma unroll
        for (int k = 0; k < W; ++k) g_M[lane][k] = g_O[lane][k] = g_L[lane][k] = 0ull;
    }

    // ---- the rounds
    for (;;) {
        bool want = false;
        if (lane < G) {
            if (o.owner) want = o.advance();
            int side = 0;
            if (want) {
                const bool tw = (o.s.meta & M_TURN_WHITE) != 0;
                const BB<W> M = pick(tw, o.s.white, o.s.black), O = pick(tw, o.s.black, o.s.white);
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    g_M[lane][k] = M.w[k];
                    g_O[lane][k] = O.w[k];
                    g_L[lane][k] = o.s.legal.w[k];
                }
                side = mode == PS_PLAY && tw ? 2 : 1;
            }
            g_want[lane] = side;
        }
        __syncthreads();
        // which rows want which network, read from LDS after the barrier: the tests below are block-uniform
        const int my = g_want[c];
        const bool want_b = __ballot(my == 1) != 0ull, want_w = __ballot(my == 2) != 0ull;
        if (!want_b && !want_w) break;
        int a_sel = -1;
        for (int k = 1; k <= 2; ++k) {
            // one network: a single pass over every wanting row; two: a pass a side that is wanted
            if (same ? k == 2 : !(k == 1 ? want_b : want_w)) continue;
            const bool mine = same ? my != 0 : my == k;
            const PlayNetSide& sd = k == 2 ? side_w : side_b;
            uint64_t key = 0;
            net_eval_tile<KS>(
                sd.geo, sd.blob, zs, lane,
                [&](int p, int v) -> uint64_t {
                    const uint64_t* src = p == 0 ? g_M[c] : (p == 1 ? g_O[c] : g_L[c]);
                    return mine ? src[v] : 0ull;
                },
                [&](int sq, int32_t z) {
                    if (mine && sq < NN && ((g_L[c][sq >> 6] >> (sq & 63)) & 1u)) {
                        const uint64_t kk = net_move_key(z, sq);
                        key = kk > key ? kk : key;
                    }
                });
            {
                const uint64_t k1 = (uint64_t)__shfl_xor((unsigned long long)key, 16);
                key = k1 > key ? k1 : key;
                const uint64_t k2 = (uint64_t)__shfl_xor((unsigned long long)key, 32);
                key = k2 > key ? k2 : key;
            }
            __syncthreads();  // the rows' priors, written by their four lanes, are read by their owners
            if (want && mine) {
                const int sample_discs = my == 2 ? side_w.sample_discs : side_b.sample_discs;
                if (popcount(o.s.black | o.s.white) < sample_discs) {
                    const auto pr = [&](int a) { return zs[net_zs_index(a, lane)]; };
                    const uint32_t u = net_move_word(rng.seed, o.id, o.ply_index());
                    a_sel = net_sample_square(NN, g_L[lane], pr, net_draw_target(u, net_prior_sum(NN, g_L[lane], pr)));
                } else {
                    a_sel = net_key_square(key);
                }
            }
            __syncthreads();  // zs and the published rows are free again
        }
        if (want) o.apply(a_sel, 0);
    }

    // ---- the boards back, the call's outputs, the tallies: the handle has a W/D/L slot per 16 boards, this block's
    o.finish(boards, meta, legal, plies_out, nullptr, wdl, wdl_vs, (size_t)blockIdx.x);
}

}  // namespace oth_dev
#endif
