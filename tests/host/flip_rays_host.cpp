// Host build of OneWord<N>::flip_fills (csrc/bitboard.hpp: update_board's flips
// from the legal scan's fills and shifted ray constants, the code the play
// kernels run) for tests/test_flip_rays_host.py: as a shared library with C
// linkage, and, with -DFLIP_RAYS_MAIN, as a stand-alone program for
// -fsanitize=undefined that calls it for every a in [-2, 66] (a shift by 64 or
// more, or by a negative count, is what that catches).  Test infrastructure only.
#include <stdint.h>
#include <stdio.h>

#include "../../gymothelloenv_amd/csrc/bitboard.hpp"

using namespace oth;

// the eight fills of mover P against O: from legal_moves_fills (the Kogge-Stone
// scan on both axes directions) or from OneWord::legal (the kernels' dword scan,
// horizontal axis by carries)
template <int N>
static uint64_t fills_of(uint64_t P, uint64_t O, int scan, uint64_t t[8]) {
    if (scan == 0) {
        BB<1> Pb, Ob, tb[8];
        Pb.w[0] = P;
        Ob.w[0] = O;
        const BB<1> L = legal_moves_fills<N>(Pb, Ob, tb);
        for (int d = 0; d < 8; ++d) t[d] = tb[d].w[0];
        return L.w[0];
    }
    return OneWord<N>::legal(P, O, t);
}

// out[e * N*N + a] = the flips of a move on a, for every empty square a (0 on occupied ones)
template <int N>
static void flip_all_n(int E, const uint64_t* mover, const uint64_t* opp, int scan, uint64_t* legal, uint64_t* out) {
    for (int e = 0; e < E; ++e) {
        uint64_t t[8];
        legal[e] = fills_of<N>(mover[e], opp[e], scan, t);
        for (int a = 0; a < N * N; ++a) {
            const bool empty = !(((mover[e] | opp[e]) >> a) & 1ull);
            out[(size_t)e * N * N + a] = empty ? OneWord<N>::flip_fills(t, a) : 0ull;
        }
    }
}

extern "C" int host_flip_fills_all(int n, int E, const uint64_t* mover, const uint64_t* opp, int scan, uint64_t* legal,
                                   uint64_t* out) {
    switch (n) {
        case 4: flip_all_n<4>(E, mover, opp, scan, legal, out); break;
        case 5: flip_all_n<5>(E, mover, opp, scan, legal, out); break;
        case 6: flip_all_n<6>(E, mover, opp, scan, legal, out); break;
        case 7: flip_all_n<7>(E, mover, opp, scan, legal, out); break;
        case 8: flip_all_n<8>(E, mover, opp, scan, legal, out); break;
        default: return -1;
    }
    return 0;
}

#ifdef FLIP_RAYS_MAIN
static uint64_t xs = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {
    xs ^= xs << 13;
    xs ^= xs >> 7;
    xs ^= xs << 17;
    return xs;
}

// every a in [-2, 66], valid or not, on boards of three densities; the flips of a
// square of the board stay on the board and inside the opponent's discs
template <int N>
static int run_size() {
    constexpr uint64_t BD = Geo<N>::BOARD.w[0];
    for (int i = 0; i < 3000; ++i) {
        const uint64_t occ = (i % 3 == 0 ? next_u64() & next_u64() : (i % 3 == 1 ? next_u64() : next_u64() | next_u64())) & BD;
        const uint64_t P = occ & next_u64(), O = occ & ~P;
        for (int scan = 0; scan < 2; ++scan) {
            uint64_t t[8];
            (void)fills_of<N>(P, O, scan, t);
            for (int a = -2; a <= 66; ++a) {
                const uint64_t f = OneWord<N>::flip_fills(t, a);
                if (a >= 0 && a < N * N && (f & ~O)) {
                    fprintf(stderr, "FAILED n=%d a=%d P=%llx O=%llx\n", N, a, (unsigned long long)P, (unsigned long long)O);
                    return 1;
                }
            }
        }
    }
    return 0;
}

int main() {
    if (run_size<4>() || run_size<5>() || run_size<6>() || run_size<7>() || run_size<8>()) return 1;
    printf("flip_fills under UBSan: N = 4..8, a = -2..66 clean\n");
    return 0;
}
#endif
