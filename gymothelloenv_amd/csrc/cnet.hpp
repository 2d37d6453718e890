// cnet.hpp -- oth_cnet_blob_bytes / oth_cnet_pack / oth_cnet_eval: the int8 residual convolutional
// policy-value network of include/othello_mi355x.h (the spec is the header's comment on the convolutional
// network: every output is an integer function of the row, the parameters and the weight bytes).
//
// Plain host/device code, like net.hpp: the geometry of the packed weights, the pack step, and one row
// evaluated from the packed weights (cnet_row: the host definition, which reads the bytes the kernel reads).
// tests/host/cnet_host.cpp compiles it with g++; the device kernel (cnet_dev.hpp, cnet.hip) takes its layout
// from the same text, its per-element steps (net_clip, net_value, net_exp, net_prior, NET_EXP2) from net.hpp,
// and does the sums on the matrix cores.
//
// The packed weights ("blob"), in bytes, every part a multiple of 16:
//   [0, 32)    tag0 (the geometry), tag1 (shift_stem, shift_head, policy_shift, value_shift), then the 16
//              block shifts, a byte each (0 behind 2 B)
//   stem:      b int32[C], then C/16 tiles (one k-step: k = 9 i + 3 ky + kx < 27, zero weights behind)
//   conv l:    b int32[C], then C/16 x 9 x C/64 tiles: tile (T, tap, s) is number (9 T + tap) C/64 + s,
//              tap = 3 ky + kx, k = 64 s + .. the input channel                          (0 <= l < 2 B)
//   head:      b int32[16], then 9 x C/64 tiles (one output tile)
//   value:     wv int8[nn][16]: byte j of square a is wv[a][j - 1], byte 0 is 0 (head output 0 is the logit);
//              then bv int32 and 12 bytes of zero
// A tile is the A operand of one v_mfma_i32_16x16x64_i8: 64 lanes x 16 bytes, lane 16 g + r byte j =
// w[16 T + r][k = 16 g + j] of the tile's tap and k-step.  The B operand holds k = 16 g + j on the same (g, j),
// so the order in which the instruction walks k does not show in a sum; the C/D map leaves channels 16 T + 4 g
// + r of a square in natural order, so no permutation of k is needed between layers.
#pragma once
#include "net.hpp"

namespace oth {

constexpr int CNET_MAX_BLOCKS = 8, CNET_HEAD_OUT = 16, CNET_HEAD_BYTES = 32, CNET_STEM_K = 27;

// struct oth_cnet_params, restated for the host build (cnet.hip asserts the match)
struct CnetParams {
    int32_t channels, blocks, shift_stem, shift[16], shift_head, policy_shift, value_shift;
};

// a network's geometry and shifts: what the kernel takes by value
struct CnetGeo {
    int32_t n, nn, W, C, B;
    int32_t KS, OT, ST;  // k-steps of a conv (C / 64), its output tiles (C / 16), the square tiles of a board
    int32_t NP, P2;      // the padded board's side (n + 2) and squares
    int32_t shift_stem, shift_head, policy_shift, value_shift;
    uint8_t shifts[16];
    OTH_HD uint64_t stem_bytes() const { return 4u * (uint64_t)C + (uint64_t)NET_TILE_BYTES * (uint64_t)OT; }
    OTH_HD uint64_t conv_bytes() const {
        return 4u * (uint64_t)C + (uint64_t)NET_TILE_BYTES * (uint64_t)OT * 9u * (uint64_t)KS;
    }
    OTH_HD uint64_t head_bytes() const { return 64u + (uint64_t)NET_TILE_BYTES * 9u * (uint64_t)KS; }
    // where a part's biases begin; its tiles follow them
    OTH_HD uint64_t off_stem() const { return CNET_HEAD_BYTES; }
    OTH_HD uint64_t off_conv(int l) const { return off_stem() + stem_bytes() + (uint64_t)l * conv_bytes(); }
    OTH_HD uint64_t off_head() const { return off_conv(2 * B); }
    OTH_HD uint64_t off_wv() const { return off_head() + head_bytes(); }
    OTH_HD uint64_t off_bv() const { return off_wv() + 16u * (uint64_t)nn; }
    OTH_HD uint64_t bytes() const { return off_bv() + 16u; }
    OTH_HD uint64_t tag0() const {
        return 0x636e657400000000ull ^ ((uint64_t)(uint32_t)n << 24) ^ ((uint64_t)(uint32_t)B << 16) ^ (uint64_t)(uint32_t)C;
    }
    OTH_HD uint64_t tag1() const {
        return 0x6373686600000000ull ^ ((uint64_t)(uint32_t)shift_stem << 24) ^ ((uint64_t)(uint32_t)shift_head << 16) ^
               ((uint64_t)(uint32_t)policy_shift << 8) ^ (uint64_t)(uint32_t)value_shift;
    }
    // the 32 bytes a blob of this geometry and these shifts begins with
    OTH_HD void head(uint8_t* out) const {
        const uint64_t tags[2] = {tag0(), tag1()};
        for (int i = 0; i < 16; ++i) out[i] = (uint8_t)(tags[i / 8] >> (8 * (i % 8)));
        for (int i = 0; i < 16; ++i) out[16 + i] = shifts[i];
    }
};

// NULL, or what is out of range
inline const char* cnet_check(int n, const CnetParams* p) {
    if (!p) return "params is NULL";
    if (n < 4 || n > 16) return "board_size must be in [4, 16]";
    if (p->channels != 64 && p->channels != 128) return "channels must be 64 or 128";
    if (p->blocks < 1 || p->blocks > CNET_MAX_BLOCKS) return "blocks must be in [1, 8]";
    if (p->shift_stem < 0 || p->shift_stem > NET_MAX_SHIFT) return "shift_stem must be in [0, 24]";
    for (int l = 0; l < 2 * p->blocks; ++l)
        if (p->shift[l] < 0 || p->shift[l] > NET_MAX_SHIFT) return "every shift must be in [0, 24]";
    if (p->shift_head < 0 || p->shift_head > NET_MAX_SHIFT) return "shift_head must be in [0, 24]";
    if (p->policy_shift < 0 || p->policy_shift > NET_MAX_SHIFT) return "policy_shift must be in [0, 24]";
    if (p->value_shift < 0 || p->value_shift > NET_MAX_SHIFT) return "value_shift must be in [0, 24]";
    return nullptr;
}

// (of checked arguments)
inline CnetGeo cnet_geo(int n, const CnetParams& p) {
    CnetGeo g;
    g.n = n;
    g.nn = n * n;
    g.W = (n * n + 63) / 64;
    g.C = p.channels;
    g.B = p.blocks;
    g.KS = p.channels / 64;
    g.OT = p.channels / 16;
    g.ST = (n * n + 15) / 16;
    g.NP = n + 2;
    g.P2 = (n + 2) * (n + 2);
    g.shift_stem = p.shift_stem;
    g.shift_head = p.shift_head;
    g.policy_shift = p.policy_shift;
    g.value_shift = p.value_shift;
    for (int l = 0; l < 16; ++l) g.shifts[l] = l < 2 * p.blocks ? (uint8_t)p.shift[l] : (uint8_t)0;
    return g;
}

// the weight of row r (an output of the tile) and k (0 .. 63) of a tile
OTH_HD int cnet_tile_at(int r, int k) { return ((k >> 4) * 16 + r) * 16 + (k & 15); }

// the numbers of weights and biases oth_cnet_pack reads
inline size_t cnet_weights(const CnetGeo& geo) {
    const size_t C = (size_t)geo.C;
    return C * CNET_STEM_K + 2u * (size_t)geo.B * C * C * 9u + (size_t)CNET_HEAD_OUT * C * 9u + (size_t)geo.nn * 15u;
}
inline size_t cnet_biases(const CnetGeo& geo) { return (size_t)geo.C * (1u + 2u * (size_t)geo.B) + CNET_HEAD_OUT + 1u; }

// oth_cnet_pack (of checked params): w and b as the header lays them out.  NULL, or what is out of range.
inline const char* cnet_pack(int n, const CnetParams& p, const int8_t* w, const int32_t* b, uint8_t* blob) {
    const CnetGeo geo = cnet_geo(n, p);
    const int C = geo.C;
    const size_t nb = cnet_biases(geo);
    for (size_t i = 0; i < nb; ++i)
        if (b[i] < -NET_BIAS_MAX || b[i] > NET_BIAS_MAX) return "every bias must be in [-2^30, 2^30]";
    geo.head(blob);
    // the stem
    int32_t* bias = reinterpret_cast<int32_t*>(blob + geo.off_stem());
    for (int o = 0; o < C; ++o) bias[o] = b[o];
    int8_t* tile = reinterpret_cast<int8_t*>(blob + geo.off_stem() + 4u * (size_t)C);
    for (int T = 0; T < geo.OT; ++T, tile += NET_TILE_BYTES)
        for (int r = 0; r < 16; ++r)
            for (int k = 0; k < 64; ++k)
                tile[cnet_tile_at(r, k)] = k < CNET_STEM_K ? w[(size_t)(16 * T + r) * CNET_STEM_K + k] : (int8_t)0;
    w += (size_t)C * CNET_STEM_K;
    b += C;
    // the 2 B convs of the blocks, then the head (one output tile)
    for (int l = 0; l <= 2 * geo.B; ++l) {
        const bool head = l == 2 * geo.B;
        const int outs = head ? CNET_HEAD_OUT : C;
        bias = reinterpret_cast<int32_t*>(blob + (head ? geo.off_head() : geo.off_conv(l)));
        for (int o = 0; o < outs; ++o) bias[o] = b[o];
        tile = reinterpret_cast<int8_t*>(bias + outs);
        for (int T = 0; T < outs / 16; ++T)
            for (int tap = 0; tap < 9; ++tap)
                for (int s = 0; s < geo.KS; ++s, tile += NET_TILE_BYTES)
                    for (int r = 0; r < 16; ++r)
                        for (int k = 0; k < 64; ++k)
                            tile[cnet_tile_at(r, k)] = w[((size_t)(16 * T + r) * C + (size_t)(64 * s + k)) * 9u + tap];
        w += (size_t)outs * C * 9u;
        b += outs;
    }
    int8_t* wv = reinterpret_cast<int8_t*>(blob + geo.off_wv());
    for (int a = 0; a < geo.nn; ++a)
        for (int j = 0; j < 16; ++j) wv[16 * a + j] = j ? w[(size_t)a * 15u + (size_t)(j - 1)] : (int8_t)0;
    int32_t* bv = reinterpret_cast<int32_t*>(blob + geo.off_bv());
    bv[0] = b[0];
    bv[1] = bv[2] = bv[3] = 0;
    return nullptr;
}

// acc[o] (o < 16 tiles) of square (y, x): bias + the 3 x 3 taps over src, uint8 [nn][C], 0 off the board
inline void cnet_conv_at(const CnetGeo& geo, const uint8_t* part, int tiles, const uint8_t* src, int y, int x,
                         int32_t* acc) {
    const int32_t* bias = reinterpret_cast<const int32_t*>(part);
    const int8_t* tile0 = reinterpret_cast<const int8_t*>(bias + 16 * tiles);
    const int n = geo.n, C = geo.C;
    for (int o = 0; o < 16 * tiles; ++o) {
        int32_t sum = bias[o];
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            if (yy < 0 || yy >= n || xx < 0 || xx >= n) continue;
            const uint8_t* in = src + (size_t)(yy * n + xx) * C;
            for (int s = 0; s < geo.KS; ++s) {
                const int8_t* tile = tile0 + (size_t)(((o / 16) * 9 + tap) * geo.KS + s) * NET_TILE_BYTES;
                for (int g = 0; g < 4; ++g) {
                    const int8_t* wr = tile + (g * 16 + o % 16) * 16;
                    const uint8_t* ir = in + 64 * s + 16 * g;
                    for (int j = 0; j < 16; ++j) sum += (int32_t)wr[j] * (int32_t)ir[j];
                }
            }
        }
        acc[o] = sum;
    }
}

// One row from the packed weights: priors int32[nn], value, logits int32[nn + 1] or NULL.  A blob of another
// geometry or other shifts writes nothing (false).
inline bool cnet_row(const CnetGeo& geo, const uint8_t* blob, const uint64_t* boards, uint16_t meta,
                     const uint64_t* legal, int32_t* priors, int32_t* value, int32_t* logits) {
    uint8_t want[CNET_HEAD_BYTES];
    geo.head(want);
    for (int i = 0; i < CNET_HEAD_BYTES; ++i)
        if (blob[i] != want[i]) return false;
    const int n = geo.n, nn = geo.nn, C = geo.C;
    const uint64_t* plane[3] = {boards + ((meta & 1u) ? geo.W : 0), boards + ((meta & 1u) ? 0 : geo.W), legal};
    uint8_t h[256 * 128], t[256 * 128];
    int32_t acc[128], z[257];
    // the stem: 27 inputs a square
    {
        const int32_t* bias = reinterpret_cast<const int32_t*>(blob + geo.off_stem());
        const int8_t* tiles = reinterpret_cast<const int8_t*>(bias + C);
        for (int a = 0; a < nn; ++a) {
            int32_t in[CNET_STEM_K];
            for (int k = 0; k < CNET_STEM_K; ++k) {
                const int yy = a / n + (k % 9) / 3 - 1, xx = a % n + k % 3 - 1;
                const int sq = yy * n + xx;
                in[k] = yy < 0 || yy >= n || xx < 0 || xx >= n ? 0 : (int32_t)((plane[k / 9][sq >> 6] >> (sq & 63)) & 1u);
            }
            for (int o = 0; o < C; ++o) {
                int32_t sum = bias[o];
                for (int k = 0; k < CNET_STEM_K; ++k)
                    sum += (int32_t)tiles[(size_t)(o / 16) * NET_TILE_BYTES + cnet_tile_at(o % 16, k)] * in[k];
                h[(size_t)a * C + o] = (uint8_t)net_clip(sum, geo.shift_stem);
            }
        }
    }
    for (int k = 0; k < geo.B; ++k) {
        for (int a = 0; a < nn; ++a) {
            cnet_conv_at(geo, blob + geo.off_conv(2 * k), geo.OT, h, a / n, a % n, acc);
            for (int o = 0; o < C; ++o) t[(size_t)a * C + o] = (uint8_t)net_clip(acc[o], geo.shifts[2 * k]);
        }
        for (int a = 0; a < nn; ++a) {
            cnet_conv_at(geo, blob + geo.off_conv(2 * k + 1), geo.OT, t, a / n, a % n, acc);
            for (int o = 0; o < C; ++o) {
                const int32_t v = (acc[o] >> geo.shifts[2 * k + 1]) + (int32_t)h[(size_t)a * C + o];
                h[(size_t)a * C + o] = (uint8_t)(v < 0 ? 0 : (v > 127 ? 127 : v));
            }
        }
    }
    const int8_t* wv = reinterpret_cast<const int8_t*>(blob + geo.off_wv());
    int32_t zv = *reinterpret_cast<const int32_t*>(blob + geo.off_bv());
    for (int a = 0; a < nn; ++a) {
        cnet_conv_at(geo, blob + geo.off_head(), 1, h, a / n, a % n, acc);
        z[a] = acc[0];
        for (int j = 1; j < CNET_HEAD_OUT; ++j) zv += (int32_t)wv[16 * a + j] * net_clip(acc[j], geo.shift_head);
    }
    z[nn] = zv;
    if (logits)
        for (int o = 0; o <= nn; ++o) logits[o] = z[o];
    *value = net_value(zv, geo.value_shift);
    bool any = false;
    int32_t m = INT32_MIN;
    for (int a = 0; a < nn; ++a)
        if ((legal[a >> 6] >> (a & 63)) & 1u) {
            any = true;
            m = z[a] > m ? z[a] : m;
        }
    uint64_t S = 0;
    for (int a = 0; a < nn; ++a) {
        priors[a] = any && ((legal[a >> 6] >> (a & 63)) & 1u) ? (int32_t)net_exp(m, z[a], geo.policy_shift) : 0;
        S += (uint64_t)priors[a];
    }
    for (int a = 0; a < nn; ++a) priors[a] = any ? net_prior((uint32_t)priors[a], S) : 0;
    return true;
}

}  // namespace oth
