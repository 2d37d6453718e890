// net.hpp -- oth_net_blob_bytes / oth_net_pack / oth_net_eval: the int8 policy-value
// MLP of include/othello_mi355x.h (the spec is the header's comment on the network:
// every output is an integer function of the row, the parameters and the weight
// bytes).
//
// The part outside __HIPCC__ is plain host/device code: the geometry of the packed
// weights, the pack step, and one row's features, layers, head and integer softmax
// read from the packed weights.  tests/host/net_host.cpp compiles it with g++; the
// device kernel (below, net.hip's) takes its layout and its per-element steps
// (net_clip, net_value, net_exp, net_prior, the k maps) from the same text and does
// the sums on the matrix cores.
//
// The packed weights ("blob"), in bytes, every part a multiple of 16:
//   [0, 16)    two tags: the geometry and the shifts the blob was packed for
//   layer 0:   b[0] int32[H], then H/16 x 3W tiles
//   layer l:   b[l] int32[H], then H/16 x H/64 tiles            (1 <= l < L)
//   head:      bh int32[16 OT] (zero behind nn), then OT x H/64 tiles, OT = ceil((nn + 1) / 16)
// A tile is the A operand of one v_mfma_i32_16x16x64_i8: 64 lanes x 16 bytes, lane
// 16 g + r byte j = w[16 T + r][k(s, g, j)] of output tile T and k-step s (tile T s
// of a layer is tile number T S + s, S the layer's k-steps).  The k maps:
//   layer 0    k-step s = plane p W + word v (p: mover, opponent, legal), byte j of
//              lane group g is bit 16 g + j of that word: feature p nn + 64 v + 16 g + j,
//              a zero weight where 64 v + 16 g + j >= nn (so bits off the board are
//              never read as anything but a factor of a zero)
//   later      k = 64 s + 16 (j >> 2) + 4 g + (j & 3): what the C/D map of the
//              previous layer leaves on lane group g (net.hip)
// Both operands of an MFMA take their k from the same (g, j), so the order in which
// the instruction walks k does not show in a sum.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>

#include "bitboard.hpp"

namespace oth {

constexpr int NET_MAX_LAYERS = 4, NET_MAX_WIDTH = 512, NET_MAX_SHIFT = 24, NET_MAX_ROWS = 1 << 24;
constexpr int32_t NET_BIAS_MAX = 1 << 30;
constexpr int NET_TILE_BYTES = 1024;  // 64 lanes x 16 bytes
constexpr int NET_HEAD_BYTES = 16;    // the two tags

// EXP2[f] = round(2^30 * 2^(-f / 256))
static constexpr uint32_t NET_EXP2[256] = {
    1073741824u, 1070838486u, 1067942999u, 1065055341u, 1062175491u, 1059303428u, 1056439131u, 1053582579u,
    1050733751u, 1047892626u, 1045059183u, 1042233401u, 1039415261u, 1036604740u, 1033801819u, 1031006477u,
    1028218693u, 1025438448u, 1022665720u, 1019900489u, 1017142735u, 1014392438u, 1011649578u, 1008914134u,
    1006186087u, 1003465416u, 1000752102u, 998046124u, 995347464u, 992656100u, 989972014u, 987295185u,
    984625594u, 981963222u, 979308048u, 976660054u, 974019220u, 971385527u, 968758955u, 966139485u,
    963527098u, 960921775u, 958323496u, 955732243u, 953147997u, 950570738u, 948000448u, 945437108u,
    942880699u, 940331203u, 937788600u, 935252872u, 932724001u, 930201967u, 927686753u, 925178340u,
    922676710u, 920181844u, 917693724u, 915212331u, 912737649u, 910269657u, 907808339u, 905353676u,
    902905651u, 900464244u, 898029440u, 895601218u, 893179563u, 890764456u, 888355878u, 885953814u,
    883558244u, 881169153u, 878786521u, 876410331u, 874040567u, 871677210u, 869320244u, 866969651u,
    864625413u, 862287515u, 859955938u, 857630665u, 855311680u, 852998965u, 850692504u, 848392279u,
    846098274u, 843810471u, 841528855u, 839253408u, 836984114u, 834720956u, 832463917u, 830212982u,
    827968132u, 825729353u, 823496627u, 821269938u, 819049271u, 816834607u, 814625932u, 812423229u,
    810226483u, 808035676u, 805850792u, 803671817u, 801498734u, 799331526u, 797170178u, 795014675u,
    792865000u, 790721137u, 788583072u, 786450787u, 784324269u, 782203500u, 780088465u, 777979150u,
    775875538u, 773777614u, 771685363u, 769598769u, 767517817u, 765442492u, 763372778u, 761308661u,
    759250125u, 757197155u, 755149737u, 753107854u, 751071493u, 749040637u, 747015274u, 744995386u,
    742980960u, 740971982u, 738968435u, 736970306u, 734977579u, 732990241u, 731008277u, 729031671u,
    727060411u, 725094480u, 723133865u, 721178552u, 719228525u, 717283772u, 715344277u, 713410026u,
    711481005u, 709557200u, 707638598u, 705725183u, 703816941u, 701913860u, 700015924u, 698123120u,
    696235434u, 694352853u, 692475362u, 690602947u, 688735596u, 686873293u, 685016026u, 683163781u,
    681316545u, 679474303u, 677637043u, 675804750u, 673977412u, 672155015u, 670337545u, 668524990u,
    666717336u, 664914570u, 663116678u, 661323648u, 659535466u, 657752119u, 655973594u, 654199878u,
    652430958u, 650666822u, 648907455u, 647152846u, 645402981u, 643657847u, 641917433u, 640181724u,
    638450708u, 636724373u, 635002706u, 633285695u, 631573326u, 629865587u, 628162466u, 626463950u,
    624770026u, 623080683u, 621395908u, 619715688u, 618040012u, 616368866u, 614702239u, 613040119u,
    611382493u, 609729349u, 608080675u, 606436459u, 604796689u, 603161352u, 601530438u, 599903933u,
    598281827u, 596664106u, 595050760u, 593441776u, 591837143u, 590236848u, 588640881u, 587049229u,
    585461881u, 583878825u, 582300049u, 580725543u, 579155293u, 577589290u, 576027521u, 574469975u,
    572916640u, 571367506u, 569822560u, 568281792u, 566745190u, 565212742u, 563684439u, 562160268u,
    560640218u, 559124278u, 557612438u, 556104685u, 554601009u, 553101399u, 551605844u, 550114332u,
    548626854u, 547143398u, 545663953u, 544188508u, 542717053u, 541249576u, 539786068u, 538326517u,
};

// struct oth_net_params, restated for the host build (net.hip asserts the match)
struct NetParams {
    int32_t layers, width, shift[4], policy_shift, value_shift;
};

// a network's geometry and shifts: what the kernel takes by value
struct NetGeo {
    int32_t n, nn, W, L, H;
    int32_t KS, K0S, OT;  // k-steps of a later layer (H / 64) and of layer 0 (3 W); the head's tiles
    uint32_t shifts;      // shift[l] in bits [5 l, 5 l + 5)
    int32_t policy_shift, value_shift;
    OTH_HD int shift(int l) const { return (int)((shifts >> (5 * l)) & 31u); }
    // the k-steps of layer l (l = L: the head), its output tiles, and where its biases and tiles begin
    OTH_HD int steps(int l) const { return l == 0 ? K0S : KS; }
    OTH_HD int tiles(int l) const { return l == L ? OT : H / 16; }
    OTH_HD uint64_t layer_bytes(int l) const {
        return 64u * (uint64_t)tiles(l) + (uint64_t)NET_TILE_BYTES * (uint64_t)tiles(l) * (uint64_t)steps(l);
    }
    OTH_HD uint64_t off_bias(int l) const {
        uint64_t o = NET_HEAD_BYTES;
        for (int i = 0; i < l; ++i) o += layer_bytes(i);
        return o;
    }
    OTH_HD uint64_t off_tiles(int l) const { return off_bias(l) + 64u * (uint64_t)tiles(l); }
    OTH_HD uint64_t bytes() const { return off_bias(L + 1); }
    OTH_HD uint64_t tag0() const {
        return 0x6e65740000000000ull ^ ((uint64_t)(uint32_t)n << 32) ^ ((uint64_t)(uint32_t)L << 16) ^ (uint64_t)(uint32_t)H;
    }
    OTH_HD uint64_t tag1() const {
        return 0x7773000000000000ull ^ ((uint64_t)shifts << 16) ^ ((uint64_t)(uint32_t)policy_shift << 8) ^
               (uint64_t)(uint32_t)value_shift;
    }
};

// NULL, or what is out of range
inline const char* net_check(int n, const NetParams* p) {
    if (!p) return "params is NULL";
    if (n < 4 || n > 16) return "board_size must be in [4, 16]";
    if (p->layers < 1 || p->layers > NET_MAX_LAYERS) return "layers must be in [1, 4]";
    if (p->width < 64 || p->width > NET_MAX_WIDTH || p->width % 64) return "width must be a multiple of 64 in [64, 512]";
    for (int l = 0; l < p->layers; ++l)
        if (p->shift[l] < 0 || p->shift[l] > NET_MAX_SHIFT) return "every shift must be in [0, 24]";
    if (p->policy_shift < 0 || p->policy_shift > NET_MAX_SHIFT) return "policy_shift must be in [0, 24]";
    if (p->value_shift < 0 || p->value_shift > NET_MAX_SHIFT) return "value_shift must be in [0, 24]";
    return nullptr;
}

// (of checked arguments)
inline NetGeo net_geo(int n, const NetParams& p) {
    NetGeo g;
    g.n = n;
    g.nn = n * n;
    g.W = (n * n + 63) / 64;
    g.L = p.layers;
    g.H = p.width;
    g.KS = p.width / 64;
    g.K0S = 3 * g.W;
    g.OT = (g.nn + 1 + 15) / 16;
    g.shifts = 0;
    for (int l = 0; l < p.layers; ++l) g.shifts |= (uint32_t)p.shift[l] << (5 * l);
    g.policy_shift = p.policy_shift;
    g.value_shift = p.value_shift;
    return g;
}

// the k maps: the input of layer l that byte j of lane group g of k-step s multiplies (-1: none, a zero weight)
OTH_HD int net_k0(const NetGeo& geo, int s, int g, int j) {
    const int p = s / geo.W, a = 64 * (s % geo.W) + 16 * g + j;
    return a < geo.nn ? p * geo.nn + a : -1;
}
OTH_HD int net_kh(int s, int g, int j) { return 64 * s + 16 * (j >> 2) + 4 * g + (j & 3); }
OTH_HD int net_k(const NetGeo& geo, int l, int s, int g, int j) { return l == 0 ? net_k0(geo, s, g, j) : net_kh(s, g, j); }

// the steps of one element
OTH_HD int32_t net_clip(int32_t acc, int shift) {
    const int32_t v = acc >> shift;
    return v < 0 ? 0 : (v > 127 ? 127 : v);
}
OTH_HD int32_t net_value(int32_t z, int shift) {
    const int32_t v = z >> shift;
    return v < -32768 ? -32768 : (v > 32768 ? 32768 : v);
}
// e_a of a legal square: m the largest legal logit
OTH_HD uint32_t net_exp(int32_t m, int32_t z, int policy_shift) {
    const int64_t d = ((int64_t)m - (int64_t)z) >> policy_shift;
    const int64_t i = d >> 8;
    return i >= 31 ? 0u : NET_EXP2[(int)(d & 255)] >> (int)i;
}
OTH_HD int32_t net_prior(uint32_t e, uint64_t S) { return (int32_t)((65535ull * (uint64_t)e + S / 2u) / S); }

// oth_net_pack (of checked params): w and b as the header lays them out.  NULL, or what is out of range.
inline const char* net_pack(int n, const NetParams& p, const int8_t* w, const int32_t* b, uint8_t* blob) {
    const NetGeo geo = net_geo(n, p);
    const int64_t nb = (int64_t)geo.L * geo.H + geo.nn + 1;
    for (int64_t i = 0; i < nb; ++i)
        if (b[i] < -NET_BIAS_MAX || b[i] > NET_BIAS_MAX) return "every bias must be in [-2^30, 2^30]";
    uint64_t tags[2] = {geo.tag0(), geo.tag1()};
    for (int i = 0; i < 16; ++i) blob[i] = (uint8_t)(tags[i / 8] >> (8 * (i % 8)));
    for (int l = 0; l <= geo.L; ++l) {
        const int rows = l == geo.L ? geo.nn + 1 : geo.H;      // the layer's outputs
        const int cols = l == 0 ? 3 * geo.nn : geo.H;          // ... and inputs
        int32_t* bias = reinterpret_cast<int32_t*>(blob + geo.off_bias(l));
        for (int o = 0; o < 16 * geo.tiles(l); ++o) bias[o] = o < rows ? b[o] : 0;
        int8_t* tile = reinterpret_cast<int8_t*>(blob + geo.off_tiles(l));
        for (int T = 0; T < geo.tiles(l); ++T)
            for (int s = 0; s < geo.steps(l); ++s)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 16; ++j) {
                        const int o = 16 * T + (lane & 15), k = net_k(geo, l, s, lane >> 4, j);
                        *tile++ = o < rows && k >= 0 ? w[(size_t)o * cols + k] : (int8_t)0;
                    }
        w += (size_t)rows * cols;
        b += rows;
    }
    return nullptr;
}

// One row from the packed weights: priors int32[nn], value, logits int32[nn + 1] or NULL.  A blob of another
// geometry or other shifts writes nothing (false).
inline bool net_row(const NetGeo& geo, const uint8_t* blob, const uint64_t* boards, uint16_t meta, const uint64_t* legal,
                    int32_t* priors, int32_t* value, int32_t* logits) {
    uint64_t tags[2] = {0, 0};
    for (int i = 0; i < 16; ++i) tags[i / 8] |= (uint64_t)blob[i] << (8 * (i % 8));
    if (tags[0] != geo.tag0() || tags[1] != geo.tag1()) return false;
    const uint64_t* plane[3] = {boards + ((meta & 1u) ? geo.W : 0), boards + ((meta & 1u) ? 0 : geo.W), legal};
    int32_t h[3 * 256], out[NET_MAX_WIDTH];
    for (int p = 0; p < 3; ++p)
        for (int a = 0; a < geo.nn; ++a) h[p * geo.nn + a] = (int32_t)((plane[p][a >> 6] >> (a & 63)) & 1u);
    for (int l = 0; l <= geo.L; ++l) {
        const int32_t* bias = reinterpret_cast<const int32_t*>(blob + geo.off_bias(l));
        const int8_t* tiles = reinterpret_cast<const int8_t*>(blob + geo.off_tiles(l));
        for (int o = 0; o < 16 * geo.tiles(l); ++o) {
            int32_t acc = bias[o];
            for (int s = 0; s < geo.steps(l); ++s)
                for (int g = 0; g < 4; ++g)
                    for (int j = 0; j < 16; ++j) {
                        const int k = net_k(geo, l, s, g, j);
                        const int8_t wv =
                            tiles[((size_t)((o / 16) * geo.steps(l) + s) * 64 + (size_t)(16 * g + o % 16)) * 16 + j];
                        if (k >= 0) acc += (int32_t)wv * h[k];
                    }
            out[o] = acc;
        }
        if (l < geo.L)
            for (int o = 0; o < geo.H; ++o) h[o] = net_clip(out[o], geo.shift(l));
    }
    if (logits)
        for (int o = 0; o <= geo.nn; ++o) logits[o] = out[o];
    *value = net_value(out[geo.nn], geo.value_shift);
    bool any = false;
    int32_t m = INT32_MIN;
    for (int a = 0; a < geo.nn; ++a)
        if ((legal[a >> 6] >> (a & 63)) & 1u) {
            any = true;
            m = out[a] > m ? out[a] : m;
        }
    uint64_t S = 0;
    for (int a = 0; a < geo.nn; ++a) {
        priors[a] = any && ((legal[a >> 6] >> (a & 63)) & 1u) ? (int32_t)net_exp(m, out[a], geo.policy_shift) : 0;
        S += (uint64_t)priors[a];
    }
    for (int a = 0; a < geo.nn; ++a) priors[a] = any ? net_prior((uint32_t)priors[a], S) : 0;
    return true;
}

}  // namespace oth
