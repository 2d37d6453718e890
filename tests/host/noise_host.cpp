// Host build of the root noise (csrc/noise.hpp: whether a board takes noise, a square's table
// draw and one row's two passes -- the text the device kernel runs on a lane a board, compiled
// with g++) for tests/test_noise_host.py: a shared library with C linkage that has
// oth_puct_noise on host memory.  tests/host/noise_san_main.cpp includes this file under
// -fsanitize=address,undefined.  Test infrastructure only.
#include <stdint.h>

#include "../../gymothelloenv_amd/csrc/noise.hpp"

using namespace oth;

// 0, 1 for arguments out of range (nothing is written).  handle_boards uint64[E][2W] and
// handle_legal uint64[E][W]: the handle's; id0: id_key + env_id_base; the rest as oth_puct_noise.
extern "C" int host_puct_noise(int n, int E, int K, const uint64_t* handle_boards, const uint64_t* handle_legal,
                               const uint8_t* kind, const uint64_t* boards, const int32_t* in, int32_t* out,
                               int32_t epsilon, const uint32_t* table, uint64_t seed, uint32_t id0, uint64_t counter) {
    if (n < 4 || n > 16 || E < 1 || K < 1 || K > 64 || !in || !out || !table || (kind == nullptr) != (boards == nullptr) ||
        epsilon < 0 || epsilon > NOISE_MAX_EPSILON)
        return 1;
    const int nn = n * n, W = (nn + 63) / 64;
    for (int e = 0; e < E; ++e)
        noise_board(nn, W, K, (size_t)e, handle_boards, handle_legal, kind, boards, in, out, epsilon, table, seed,
                    id0 + (uint32_t)e, counter);
    return 0;
}
