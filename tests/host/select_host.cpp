// Host build of select64_tab (csrc/bitboard.hpp: the k-th set bit of a word by
// sign masks, the bit inside its byte from the sel8 table -- the play kernels'
// pick) for tests/test_select_host.py: a stand-alone program, built plain and
// with -fsanitize=undefined, that checks it against select64 (the nibble form)
// for every k < popcount of every word below.  Test infrastructure only.
#include <stdint.h>
#include <stdio.h>

#include "../../gymothelloenv_amd/csrc/bitboard.hpp"

using namespace oth;

static uint64_t tab[256];  // the table as k_play_rand stages it in LDS
static unsigned long long words = 0, picks = 0;

static uint64_t xs = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {
    xs ^= xs << 13;
    xs ^= xs >> 7;
    xs ^= xs << 17;
    return xs;
}

// every rank of x; 0 when both forms agree and name the k-th set bit
static int check(uint64_t x) {
    const uint8_t* sel8 = reinterpret_cast<const uint8_t*>(tab);
    const int n = popc64(x);
    uint64_t rest = x;
    for (int k = 0; k < n; ++k) {
        const int want = __builtin_ctzll(rest);  // the k-th set bit, ascending
        rest &= rest - 1;
        const int ref = select64(x, k), got = select64_tab(x, k, sel8);
        if (ref != want || got != want) {
            fprintf(stderr, "FAILED x=%016llx k=%d: k-th bit %d, select64 %d, select64_tab %d\n", (unsigned long long)x, k,
                    want, ref, got);
            return 1;
        }
    }
    ++words;
    picks += (unsigned long long)n;
    return 0;
}

// a byte with c set bits, drawn
static uint64_t byte_with(int c) {
    uint64_t b = 0;
    while (popc64(b) < c) b |= 1ull << (next_u64() % 8);
    return b;
}

int main() {
    for (int i = 0; i < 256; ++i) tab[i] = sel8_word((uint32_t)i);
    // all 2^16 patterns in each 16-bit quarter, alone and over a drawn background
    // in the other quarters (the ranks below and above the quarter's)
    for (int q = 0; q < 4; ++q)
        for (uint64_t p = 0; p < 65536; ++p) {
            const uint64_t bg = next_u64() & ~(0xFFFFull << (16 * q));
            if (check(p << (16 * q)) || check((p << (16 * q)) | bg)) return 1;
        }
    // every single-bit word, every word with one bit missing, the full word
    for (int b = 0; b < 64; ++b)
        if (check(1ull << b) || check(~(1ull << b))) return 1;
    if (check(~0ull)) return 1;
    // byte-prefix counts on both sides of every k: each byte empty, with 1, 2 or 7
    // bits, or full, in every combination (5^8 words), so that k meets every prefix
    // count q with k = q - 1, q and q + 1, empty and full bytes beside it
    static const int counts[5] = {0, 1, 2, 7, 8};
    for (int c = 0; c < 390625; ++c) {
        uint64_t x = 0;
        for (int b = 0, r = c; b < 8; ++b, r /= 5) x |= byte_with(counts[r % 5]) << (8 * b);
        if (check(x)) return 1;
    }
    // 10^6 drawn words: sparse, even and dense
    for (int i = 0; i < 1000000; ++i) {
        const uint64_t a = next_u64(), b = next_u64();
        if (check(i % 3 == 0 ? a & b : (i % 3 == 1 ? a : a | b))) return 1;
    }
    printf("select64_tab == select64 == the k-th set bit: %llu words, %llu picks clean\n", words, picks);
    return 0;
}
