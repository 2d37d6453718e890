// playouts_n.hip -- k_playouts (oth_playouts: Monte-Carlo playouts per board or
// per legal move, playouts.hpp) in a translation unit of its own per board
// size (-DOTH_N=4 .. 16), so that it can carry its own scheduler flags
// (build.py PLAYOUT_FLAGS) without touching the rest of the library.
#include "playouts.hpp"
#include "launch.hpp"

#ifndef OTH_N
#error "compile with -DOTH_N=<board size>"
#endif

using namespace oth;
using namespace oth_dev;

namespace oth_host {

// blocks in flight to aim for where one board's playouts are split: 256 CUs x 8
constexpr long long PLAYOUT_TARGET_BLOCKS = 2048;

template <int N>
int launch_playouts(oth_env* env, int mode, int R, uint64_t seed, uint32_t id_key, uint64_t counter, int32_t* wdl,
                    int32_t* score, int32_t* best, hipStream_t st) {
    constexpr int NN = N * N;
    const long long E = env->E;
    int EPB = 1;
    long long chunks;  // 256-lane chunks of one group's tasks
    if (mode == OTH_PLAYOUT_ROOT) {
        if (R < BLOCK) EPB = BLOCK / R;
        chunks = ((long long)EPB * R + BLOCK - 1) / BLOCK;
    } else {
        // the board's legal count is device data: size B for a middle game's upper range;
        // a board with more moves loops, one with fewer leaves blocks that find no task
        const int k_est = NN - 4 < 24 ? NN - 4 : 24;
        chunks = ((long long)k_est * R + BLOCK - 1) / BLOCK;
    }
    const long long groups = (E + EPB - 1) / EPB;
    long long B = PLAYOUT_TARGET_BLOCKS / groups;
    if (B > chunks) B = chunks;
    if (B < 1) B = 1;
    const int split = B > 1;
    const size_t rows = mode == OTH_PLAYOUT_ROOT ? (size_t)E : (size_t)E * NN;
    if (split)  // the blocks of a group add into zeroed outputs
        launch_k(k_playout_zero<N>, dim3((unsigned)((rows * 3 + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, wdl, rows * 3,
                 score, rows);
    const PlayoutKey key{seed, counter * 64u, id_key, env->id_base};
    const dim3 grid((unsigned)(groups * B)), block(BLOCK);
    if (mode == OTH_PLAYOUT_ROOT)
        launch_k((k_playouts<N, OTH_PLAYOUT_ROOT>), grid, block, 0, st, env->boards, env->meta, env->legal, env->E, R,
                 EPB, (int)B, key, wdl, score, split, env->tables);
    else
        launch_k((k_playouts<N, OTH_PLAYOUT_MOVES>), grid, block, 0, st, env->boards, env->meta, env->legal, env->E, R,
                 EPB, (int)B, key, wdl, score, split, env->tables);
    if (best)  // from the finished counts (a board's playouts may be split over blocks): a launch of its own
        launch_k(k_playout_best<N>, dim3((unsigned)((E + BLOCK - 1) / BLOCK)), block, 0, st, env->meta, env->legal,
                 env->E, wdl, best);
    return after_launch("oth_playouts");
}

template int launch_playouts<OTH_N>(oth_env*, int, int, uint64_t, uint32_t, uint64_t, int32_t*, int32_t*,
                                    int32_t*, hipStream_t);

}  // namespace oth_host
