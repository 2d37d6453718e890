// noise.hip -- k_puct_noise (oth_puct_noise: Dirichlet root noise mixed into rows of priors, noise.hpp) in one
// translation unit for every board size: N and W are run-time values.
//
// A lane a board, as k_puct_pick: the lane reads its board of the handle (leaf mode: and its first row's kind
// and leaf board), walks the legal squares twice -- the sum of the table draws, then the division -- and writes
// the mixed squares; one Philox block serves four squares, and the second pass draws the blocks again, so
// nothing is kept between the passes but the sum: no scratch, no LDS.  The call runs once or twice a move.
#include "noise.hpp"
#include "launch.hpp"
#include "state.hpp"

using namespace oth;

static_assert(NOISE_TABLE == OTH_NOISE_TABLE && NOISE_G_MAX == OTH_NOISE_G_MAX &&
                  NOISE_LEAF_EXPAND == OTH_PUCT_LEAF_EXPAND,
              "the header's limits");
static_assert(NOISE_RNG == oth_dev::RNG_PUCT_NOISE, "state.hpp's purpose word");

namespace oth_dev {

constexpr int NOISE_BLOCK = 64;  // one wave a block, one lane a board

__global__ __launch_bounds__(NOISE_BLOCK) void k_puct_noise(int nn, int W, int E, int K,
                                                            const uint64_t* __restrict__ handle_boards,
                                                            const uint64_t* __restrict__ handle_legal,
                                                            const uint8_t* __restrict__ kind,
                                                            const uint64_t* __restrict__ boards, const int32_t* in,
                                                            int32_t* out, int32_t epsilon,
                                                            const uint32_t* __restrict__ table, uint64_t seed,
                                                            uint32_t id0, uint64_t counter) {
    const long long e = (long long)blockIdx.x * NOISE_BLOCK + threadIdx.x;
    if (e >= E) return;
    noise_board(nn, W, K, (size_t)e, handle_boards, handle_legal, kind, boards, in, out, epsilon, table, seed,
                id0 + (uint32_t)e, counter);
}

}  // namespace oth_dev

namespace oth_host {

using namespace oth_dev;

// (of checked arguments)
int launch_puct_noise(oth_env* env, int K, const uint8_t* kind, const uint64_t* boards, const int32_t* priors_in,
                      int32_t* priors_out, int epsilon, const uint32_t* table, uint64_t seed, uint32_t id_key,
                      uint64_t counter, hipStream_t st) {
    const dim3 grid((unsigned)((env->E + NOISE_BLOCK - 1) / NOISE_BLOCK)), block(NOISE_BLOCK);
    launch_k(k_puct_noise, grid, block, 0, st, env->n * env->n, env->W, env->E, K, env->boards, env->legal, kind,
             boards, priors_in, priors_out, epsilon, table, seed, id_key + env->id_base, counter);
    return after_launch("oth_puct_noise");
}

}  // namespace oth_host
