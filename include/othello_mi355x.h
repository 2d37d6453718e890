/*
 * othello_mi355x.h -- C ABI of the MI355X-native vectorised Othello rules engine.
 *
 * Drop-in boundary for the reference's hot path: the
 * in-process Gym-style API of OthelloBaseEnv / SimpleOthelloEnv / OthelloEnv
 * (othello.py:21-501), batched over E boards that live in HBM.  The reference
 * is pure Python and has no FFI of its own, so these entry points are what a
 * ctypes binding of it would call (INTEGRATION.md shows that binding).
 *
 * Each entry point below names the reference function it replaces.
 *
 * Conventions
 *   - All array arguments are DEVICE pointers (hipMalloc / torch.cuda tensors)
 *     unless stated; `stream` is a hipStream_t (NULL = the null stream).  Calls
 *     only enqueue work: nothing synchronises the host.
 *   - Square a = row * N + col (othello.py:392-393); action a in [0, N*N).
 *   - W = ceil(N*N / 64) 64-bit words per colour (1 for N <= 8, up to 4 for N = 16).
 *   - State exchange format (also used by the test oracle):
 *       boards  uint64[E][2W]  words 0..W-1 black discs, W..2W-1 white discs
 *       meta    uint16[E]      bit0 white to move (player_turn == WHITE_DISK)
 *                              bit1 terminated
 *                              bits2-3 winner: 0 NO_DISK / draw, 1 WHITE, 2 BLACK
 *                              bits8-15 random-opening plies still to play
 *       legal   uint64[E][W]   possible_moves -- NOT recomputed on terminal
 *                              plies, exactly like the reference (othello.py:431-433)
 *   - Return value: OTH_OK (0) or a negative OTH_E* code; oth_last_error()
 *     gives the message for the calling thread.
 *   - A handle is bound to one device; calls on one handle must be serialised
 *     by the caller.  Separate handles are independent.
 */
#ifndef OTHELLO_MI355X_H
#define OTHELLO_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct oth_env oth_env;
typedef void *oth_stream_t; /* hipStream_t */

enum {
    OTH_OK = 0,
    OTH_EINVAL = -1, /* bad argument (board size outside [4,16], NULL pointer, ...) */
    OTH_EHIP = -2,   /* a HIP runtime call failed */
    OTH_ENOMEM = -3
};

/* create flags: the reference's constructor switches (othello.py:222-227) */
enum {
    OTH_SUDDEN_DEATH = 1, /* sudden_death_on_invalid_move */
    OTH_DISK_REWARD = 2,  /* num_disk_as_reward */
    OTH_AUTO_RESET = 4    /* batched only: reset an env right after its terminal ply */
};

/* on-device scripted policies (simple_policies.py): RandomPolicy, GreedyPolicy,
 * MaxiMinPolicy(max_search_depth = d) for d = 1 .. OTH_MAXIMIN_MAX_DEPTH as
 * OTH_POLICY_MAXIMIN(d); MAXIMIN1 plays exactly GREEDY's moves */
enum {
    OTH_POLICY_RANDOM = 0,
    OTH_POLICY_GREEDY = 1,
    OTH_POLICY_MAXIMIN1 = 2,
    OTH_POLICY_MAXIMIN2 = 3,
    OTH_POLICY_MAXIMIN3 = 4
};
#define OTH_MAXIMIN_MAX_DEPTH 10
#define OTH_POLICY_MAXIMIN(d) (OTH_POLICY_MAXIMIN1 + (d) - 1)
#define OTH_POLICY_LAST OTH_POLICY_MAXIMIN(OTH_MAXIMIN_MAX_DEPTH)
/* oth_policy_actions, oth_step_policy and oth_reset_vs / oth_step_vs refuse
 * MaxiMin(d >= 3) calls whose searches are estimated above this many leaves.
 * The first estimate is E x b^d x the searches per board in the call (n_plies
 * for oth_step_policy, 2 opponent replies for the _vs calls) with b = max(2,
 * N*N / 6) moves per position (8x8 middle games: ~10).  Above the budget the
 * call reads the boards (a synchronisation of `stream`; refused during a stream
 * capture) and bounds each live board's search by its own position: its
 * possible_moves at the root, then at most min(b, e - j) moves at level j for
 * e empty squares, since every level places a disc (simple_policies.py:138).
 * So late-game boards search to any depth the budget allows (one 8x8 board
 * with 10 empty squares at depth 10: <= 10! leaves).  Refused calls launch
 * nothing; split the boards over several calls or search shallower. */
#define OTH_MAXIMIN_LEAF_BUDGET 17179869184.0

/* observation layouts */
enum {
    OTH_OBS_BOARD = 0,       /* (E,N,N)   get_observation(): mover +1, opponent -1 (othello.py:363-369) */
    OTH_OBS_BOARD_LEGAL = 1, /* (E,2,N,N) get_observation() with possible_actions_in_obs (othello.py:370-376) */
    OTH_OBS_MAKE_STATE = 2,  /* (E,4,N,N) util.make_state(obs, env) planes (util.py:48-74) */
    OTH_OBS_ABSOLUTE = 3,    /* (E,N,N)   board_state: white +1, black -1 (othello.py:257) */
    OTH_OBS_LEGAL = 4        /* (E,N,N)   possible_moves as 0 / 1 (othello.py:313-343; the plane of
                                          OTH_OBS_BOARD_LEGAL alone: int8 views as a bool mask) */
};
/* observation element types; OTH_BF16 is bfloat16 (the observations' values
 * -1 / 0 / +1 are exact in it): half the bytes of float32 for a network that
 * takes bfloat16 input, e.g. make_state for a learner under bf16 autocast */
enum { OTH_I8 = 0, OTH_I32 = 1, OTH_I64 = 2, OTH_F32 = 3, OTH_F64 = 4, OTH_BF16 = 5 };

/* masked-categorical modes (oth_masked_sample) */
enum {
    OTH_MASKED_SAMPLE = 0, /* FixedCategorical(...).sample() / np.random.choice: actions out */
    OTH_MASKED_MODE = 1,   /* FixedCategorical(...).mode(): first largest legal logit; actions out */
    OTH_MASKED_EVAL = 2,   /* evaluate_actions: actions in, log-probs of those actions out */
    /* or-ed into a mode: entropy[e] = entropy of the UNMASKED categorical over
     * all N*N squares, as Policy.evaluate_actions returns it (dist.entropy(),
     * model.py:175; the caller takes the mean) instead of the masked one */
    OTH_MASKED_FULL_ENTROPY = 4
};

/* OthelloBaseEnv.__init__ (othello.py:222-254) for n_envs boards of size
 * board_size (clamped to >= 4 like othello.py:230; > 16 is OTH_EINVAL).
 * seed / env_id_base key every random draw: env i uses id env_id_base + i
 * (mod 2^32), so a sharded run reproduces an unsharded one.  Two stateless
 * functions of (seed, id, 64-bit counter, purpose) draw everything:
 *   - moves and samples: Philox4x32-10 with key (seed lo, seed hi) and counter
 *     (id, counter lo, counter hi, purpose).  Purpose 0: the random move of
 *     ply g is word g % 4 of the block with counter g / 4.  Purpose 3: the
 *     sampler's uniform is (word 0 of the block with the sample counter) >> 8,
 *     times 2^-24.
 *     Purposes 4 (oth_puct_pick), 5 (oth_replay_sample), 6 (oth_puct_noise)
 *     and 7 (the network's sampled move: oth_play_net, oth_reset_vs_net,
 *     oth_step_vs_net and their _cnet twins) are stated with those calls.
 *   - random-opening lengths: three murmur3 32-bit finalisers (fmix32),
 *       key = fmix32(seed lo ^ fmix32(seed hi ^ purpose * 0x7FEB352D)),
 *       word = fmix32(fmix32(key ^ ply lo ^ ply hi * 0x9E3779B9) ^ id),
 *     with purpose 1 at an auto-reset (the counter is the terminal ply; the
 *     call counter in oth_step_vs) and purpose 2 in oth_reset / oth_reset_vs.
 * A 32-bit word u picks index floor(u * n / 2^32) among n choices: the legal
 * moves in ascending order, or the initial_rand_steps / 2 + 1 opening lengths
 * 0, 2, ..
 * initial_rand_steps: SimpleOthelloEnv's random-opening length bound
 * (othello.py:62-63) applied by oth_reset and auto-reset.  Boards start reset. */
int oth_create(int32_t n_envs, int32_t board_size, uint32_t flags, uint64_t seed, uint32_t env_id_base,
               int32_t initial_rand_steps, int32_t device, oth_env **out);
int oth_destroy(oth_env *env);

/* OthelloBaseEnv.reset (othello.py:265-271) for every env, or only where
 * mask[e] != 0 (mask: device uint8[E] or NULL). */
int oth_reset(oth_env *env, const uint8_t *mask, oth_stream_t stream);

/* OthelloBaseEnv.step (othello.py:412-462) with external actions int32[E].
 * Out: rewards int32[E], dones uint8[E] (either may be NULL).  An env that is
 * already terminated is left unchanged and reports done = 1, reward = 0 (the
 * reference raises ValueError there, othello.py:415-416; the single-env
 * wrapper does so on the host). */
int oth_step(oth_env *env, const int32_t *actions, int32_t *rewards, uint8_t *dones, oth_stream_t stream);

/* oth_step, then the observation of the stepped boards in the same call:
 * OthelloBaseEnv.step's returned get_observation() (othello.py:462; layout
 * OTH_OBS_BOARD / OTH_OBS_BOARD_LEGAL) or any oth_observe layout / dtype into
 * obs (E, planes, N, N).  The values are exactly oth_step followed by
 * oth_observe: the state after the ply (and after an auto-reset).  One launch
 * where the board is one word and N*N % 4 == 0 with obs aligned to 4
 * elements (the observation is written from the registers that stepped the
 * board, nothing read back); two launches otherwise. */
int oth_step_observe(oth_env *env, const int32_t *actions, int32_t *rewards, uint8_t *dones, int32_t layout,
                     int32_t dtype, void *obs, oth_stream_t stream);

/* n_plies plies of on-device play: each env's mover picks with `policy`
 * (RandomPolicy.get_action simple_policies.py:37-41 / GreedyPolicy.get_action
 * :69-92, or a random move while random-opening plies remain) and steps.
 * Outputs are [n_plies][E] (any may be NULL): the action played (-1 for an
 * env that was already terminated), reward, done.  Finished games are tallied
 * into the handle's win/draw/loss counters (oth_counts). */
int oth_step_policy(oth_env *env, int32_t policy, int32_t n_plies, int32_t *actions, int32_t *rewards,
                    uint8_t *dones, oth_stream_t stream);

/* Monte-Carlo playouts from the handle's live positions (no reference
 * counterpart: the leaf evaluation of MCTS, flat Monte-Carlo move selection, a
 * cheap value target).  From each board (OTH_PLAYOUT_ROOT), or from each board
 * after each of its possible moves (OTH_PLAYOUT_MOVES), n_playouts = R games of
 * uniformly random legal moves are played to the end on private copies.
 *
 * Handle state.  The call reads boards, meta and possible_moves and writes
 * nothing of the handle: boards, meta, possible_moves, the ply counter, the
 * graph offsets and both tallies (oth_counts, oth_counts_vs) stay as they are.
 * It only enqueues work.  The handle's flags (sudden death, disk reward,
 * auto-reset) and random-opening plies left in meta play no part.
 *
 * ROOT: for each env e and r in [0, R), a copy of env e's position plays random
 *   moves until it is terminated.
 * MOVES: for each env e, each square a set in the handle's stored
 *   possible_moves[e] (not a recomputation: after oth_set_state with a narrower
 *   mask only those squares are evaluated) and each r, the copy first takes
 *   exactly oth_step's ply with action a (flags 0, no reset), then plays
 *   randomly to the end.
 *
 * Draws.  Playout ply p (p = 0 is the first RANDOM ply, after the forced move
 * of MOVES mode) draws like every random move: Philox4x32-10, purpose 0, key =
 * this call's `seed` (not the handle's), counter g = counter * 256 + p (block
 * g / 4, word g % 4); a playout has at most N*N - 4 < 256 random plies, and
 * counter >= 2^56 is OTH_EINVAL.  The id is
 *     id_key + (env_id_base + e) * S + a * R + r   (mod 2^32),
 * S = R and a = 0 in ROOT mode, S = N*N*R in MOVES mode: a function of the
 * global env id, the square and r alone, never of how playouts are mapped to
 * lanes or of how many moves are legal, so a sharded run equals the unsharded
 * one.
 *
 * Outputs (device pointers; every element is written, nothing needs zeroing):
 *   wdl    required.  ROOT int32[E][3], MOVES int32[E][N*N][3]: {wins, draws,
 *          losses} of the R playouts, counted from the side to move at the ROOT
 *          of env e.  Squares not in possible_moves and boards already
 *          terminated get zeros.
 *   score  may be NULL.  ROOT int32[E], MOVES int32[E][N*N]: the sum over the R
 *          playouts of (root mover's discs - opponent's discs) on the final board.
 *   best   may be NULL; MOVES only (non-NULL in ROOT mode is OTH_EINVAL).
 *          int32[E]: the possible move with the largest wins - losses, the
 *          lowest square on ties; -1 for a terminated board or an empty
 *          possible_moves.  Computed on the device in integers.
 * OTH_EINVAL: NULL handle, NULL wdl, unknown mode, R < 1 or R > OTH_PLAYOUTS_MAX,
 * more than 2^31 - 1 playouts in the call (E*R in ROOT mode, E*N*N*R in MOVES
 * mode).  Every board size works.
 *
 * Under a HIP-graph capture the call is capturable (it only enqueues), but it
 * bakes `counter` in: every replay repeats the same playouts.  It does not use
 * the graph regions' counter offsets (oth_graph_begin). */
enum { OTH_PLAYOUT_ROOT = 0, OTH_PLAYOUT_MOVES = 1 };
#define OTH_PLAYOUTS_MAX 65536
int oth_playouts(oth_env *env, int32_t mode, int32_t n_playouts /* R */, uint64_t seed, uint32_t id_key,
                 uint64_t counter, int32_t *wdl, int32_t *score, int32_t *best, oth_stream_t stream);

/* Exact endgame values and best moves of the handle's live positions (no
 * reference counterpart: what a position is worth, where playouts estimate).
 *
 * The value.  G(pos, mover) is the final disc difference under best play by
 * both sides, counted from mover's side, with the reference's end-of-game
 * rules (othello.py:424-442, 473-501):
 *   game end (the board is full, or neither side has a move):
 *       G = discs(mover) - discs(other): raw counts, no bonus for empty
 *       squares, the quantity oth_playouts sums in `score`; sign(G) is
 *       determine_winner from the mover's side;
 *   the mover has moves:  G = max over moves a of -G(pos after a, other);
 *   the mover has no move but the other side has (a pass):
 *       G = -G(pos, other); no disc is placed.
 * At the root the move list is the handle's stored possible_moves[e], as
 * oth_step and oth_playouts (MOVES) treat it: after oth_set_state with a
 * narrower mask only those squares are valued.  Each root move is oth_step's
 * ply with flags 0; below the root, moves are recomputed from the boards.
 *
 * Handle state.  The call writes nothing of the handle: boards, meta,
 * possible_moves, the ply counter, the graph offsets and both tallies stay as
 * they are.  It only enqueues work, never synchronises the host, is capturable
 * into a HIP graph and draws no random number.
 *
 * Outputs (device pointers; every element of every non-NULL output is written,
 * nothing needs zeroing): value int32[E] (required); best int32[E],
 * move_values int32[E][N*N], status uint8[E], nodes uint64[E] (each may be
 * NULL).  By status:
 *   TERMINATED  meta bit 1 set.  value = discs(side in the turn bit) -
 *               discs(other); best -1; move_values all OTH_SOLVE_NO_VALUE.
 *   SKIPPED     live, more than max_empties empty squares (N*N -
 *               popcount(black | white)).  value OTH_SOLVE_NO_VALUE, best -1,
 *               move_values all NO_VALUE.  No search work is launched for it.
 *   NO_MOVE     live, stored possible_moves empty: as SKIPPED.
 *   EXACT       otherwise.  move_values[a] = -G(after a, other) for every
 *               stored possible move a, NO_VALUE elsewhere; value their
 *               maximum; best the lowest square that attains it.
 *   ABORTED     some root move's search visited more than max_nodes nodes.
 *               value NO_VALUE, best -1; move_values exact for the moves that
 *               finished, NO_VALUE for the abandoned ones.
 * Nodes.  A node is a position reached by placing a disc: the root's children
 * count, a pass adds none.  nodes[e] is the sum over the board's root moves (an
 * abandoned move adds max_nodes + 1); 0 for every status but EXACT and ABORTED.
 * The budget max_nodes, in [1, 2^32 - 1], is per root move and bounds the
 * kernel's running time whatever the input.
 *
 * Determinism.  value, best, move_values, status and nodes of a board are
 * functions of that board's state and the two limits alone: not of E, the
 * board's index, its neighbours or how tasks are mapped to lanes (one lane
 * searches one root move with the full window; no bound is shared).  Two
 * calls give identical bytes.
 *
 * OTH_EINVAL: NULL handle, NULL value, max_empties outside [1,
 * OTH_SOLVE_MAX_EMPTIES], max_nodes outside its range; checked before the
 * handle is read.  Every board size works. */
#define OTH_SOLVE_MAX_EMPTIES 14
#define OTH_SOLVE_NO_VALUE (-32768)
enum { OTH_SOLVE_EXACT = 0, OTH_SOLVE_TERMINATED = 1, OTH_SOLVE_SKIPPED = 2,
       OTH_SOLVE_NO_MOVE = 3, OTH_SOLVE_ABORTED = 4 };
int oth_solve(oth_env *env, int32_t max_empties, uint64_t max_nodes,
              int32_t *value, int32_t *best, int32_t *move_values,
              uint8_t *status, uint64_t *nodes, oth_stream_t stream);

/* Depth-limited alpha-beta over a positional evaluation the caller supplies
 * (no reference counterpart: the middle game's deterministic look-ahead, where
 * oth_solve serves the last 14 empty squares; the evaluation is the "weighted
 * piece counter" plus mobility).
 *
 * The value.  M: the discs of the side to move, O: the other side's, L(M, O):
 * get_possible_actions for M against O.
 *   evaluation  H(M, O) = sum_a weights[a] ([a in M] - [a in O])
 *                         + mobility_weight (|L(M, O)| - |L(O, M)|)
 *   game end    T(M, O) = terminal_weight (|M| - |O|): raw disc counts, as oth_solve's
 * V_d(M, O), with d discs still to place, is the first rule that applies:
 *   1. game end (the board is full, or L(M, O) and L(O, M) are both empty): T(M, O);
 *   2. d == 0: H(M, O) -- also for a mover without a move: the mobility term
 *      sees it, no pass is played at the frontier;
 *   3. the mover has no move and the other side has one: -V_d(O, M); a pass
 *      places no disc and consumes no depth;
 *   4. otherwise max over a in L(M, O) of -V_{d-1}(position after a, other side).
 * At the root the move list is the handle's stored possible_moves[e] (as
 * oth_step, oth_playouts in MOVES mode and oth_solve treat it), each root move
 * is oth_step's ply with flags 0, move_values[a] = -V_{depth-1}(after a),
 * value is their maximum and best the lowest square that attains it.
 *
 * Ranges: depth in [1, OTH_SEARCH_MAX_DEPTH]; weights device int8[N*N], any
 * value, -128 included; mobility_weight in [-127, 127]; terminal_weight in
 * [1, 32767]; max_nodes in [1, 2^32 - 1], per root move.  Then |H| <= 128 * 256
 * + 127 * 256 < 2^16 and |T| <= 32767 * 256 < 2^23: every value lies strictly
 * inside (-2^24, 2^24), the bound the kernel's frames and reduction keys rely
 * on.  With depth beyond the end of the game and terminal_weight 1 the values
 * are oth_solve's.
 *
 * Outputs, nodes, determinism and handle state are oth_solve's contract (every
 * element of every non-NULL output is written; value is required, the others
 * may be NULL), with the status codes' numbers kept; code 2 (SKIPPED) never
 * occurs, any number of empty squares is searched:
 *   TERMINATED  value = terminal_weight (discs(side in the turn bit) -
 *               discs(other)); best -1; move_values all OTH_SEARCH_NO_VALUE.
 *   NO_MOVE     live, stored possible_moves empty: value NO_VALUE, best -1,
 *               move_values all NO_VALUE.
 *   DONE        move_values[a] for every stored possible move a, NO_VALUE
 *               elsewhere; value and best as above.
 *   ABORTED     some root move's search placed more than max_nodes discs:
 *               value NO_VALUE, best -1; the finished moves keep their values,
 *               the abandoned ones get NO_VALUE.
 * A node is a position reached by placing a disc; nodes[e] sums the board's
 * root moves (an abandoned move adds max_nodes + 1), 0 for TERMINATED and
 * NO_MOVE.  The search is the solver's fail-soft negamax: moves in ascending
 * squares, a node finished when best >= beta, the child's window
 * (-beta, -max(alpha, best)), a pass in place with the window negated, each
 * root move a pseudo-node with the full window.  So every output, nodes
 * included, is a function of the board, the weights and the limits alone, not
 * of E, the board's index or the lane mapping; two calls give identical bytes.
 * The call writes nothing of the handle, draws no random number, only enqueues
 * work and is capturable into a HIP graph.
 *
 * OTH_EINVAL: NULL handle, NULL value, NULL weights, a limit out of range;
 * checked before the handle is read.  Every board size works. */
#define OTH_SEARCH_MAX_DEPTH 14
#define OTH_SEARCH_NO_VALUE INT32_MIN
enum { OTH_SEARCH_DONE = 0, OTH_SEARCH_TERMINATED = 1, OTH_SEARCH_NO_MOVE = 3, OTH_SEARCH_ABORTED = 4 };
int oth_search(oth_env *env, int32_t depth, const int8_t *weights, int32_t mobility_weight,
               int32_t terminal_weight, uint64_t max_nodes, int32_t *value, int32_t *best,
               int32_t *move_values, uint8_t *status, uint64_t *nodes, oth_stream_t stream);

/* Monte-Carlo tree search per board (no reference counterpart: the rung after
 * oth_playouts' flat Monte-Carlo): a UCT-style tree whose leaves are evaluated
 * by random playouts, one launch for all boards, the tree in a workspace the
 * caller supplies.  Every output is defined in integers below; the mapping to
 * lanes shows in none of them.
 *
 * Parameters (struct oth_mcts_params, host memory, read during the call and
 * baked into the launch): I iterations, R playouts per evaluated node, the
 * exploration constant C in 1/256, T node slots per board, and the Philox key
 * (seed, id_key, counter) of the playouts -- not the handle's.
 *
 * The tree.  A node holds a position as oth_step with flags 0 leaves it: both
 * colours' discs, the side to move and the terminated bit.  A pass is already
 * resolved in it: after a move whose reply is a pass the same colour is to move
 * in the child.  A node also holds
 *   v  the iterations that went through it, and
 *   w  the sum, over the playouts backed up through it, of 2 [won] + [drawn],
 *      counted for the colour that moved into the node -- the side that
 *      chooses among it and its siblings.  No sign is flipped anywhere, passes
 *      included.
 * Node 0 is the board's position and used = 1.  The root's move list is the
 * handle's stored possible_moves[e], as oth_step, oth_playouts (MOVES) and
 * oth_solve treat it; below the root, moves are recomputed from the discs.
 *
 * Iteration i = 0 .. I-1 starts with cur = the root:
 *  1. Descend.  Repeat:
 *       - cur is terminated: stop.
 *       - k = cur's move count.  If cur has no reservation yet: if used + k > T,
 *         cur stays a leaf for the rest of the call: stop.  Otherwise it
 *         reserves the k consecutive slots used .. used+k-1 for its children in
 *         ascending square order, and used += k.
 *       - cur has made fewer than k children: make the next one -- the lowest
 *         square not yet made, oth_step's ply with flags 0 -- in its reserved
 *         slot, move to it and stop.
 *       - otherwise move to the child c of the largest key, the lowest square
 *         among equal keys:
 *           key = floor(2^15 w_c / (v_c R)) + floor(C isqrt(2^16 v_p) / (1 + v_c))
 *         v_p is cur's v before this iteration's backup (for the root, i);
 *         isqrt is the exact integer floor square root.  Everything fits 64-bit
 *         integers: w_c <= 2^23, C isqrt(..) < 2^32; v_c >= 1 always, since a
 *         node is evaluated in the iteration that makes it.  T >= N*N guarantees
 *         that the root can always reserve.
 *  2. Evaluate cur with R playouts.  Playout r is exactly one ROOT-mode playout
 *     of oth_playouts started from cur's position: uniformly random legal moves
 *     to the end, the same pass and game-end handling.  Playout ply p draws
 *     Philox4x32-10, purpose 0, key `seed`, counter g = counter * 256 + p (word
 *     g % 4 of block g / 4), with the id
 *         id_key + ((env_id_base + e) I + i) R + r   (mod 2^32),
 *     a function of the global env id, the iteration and r alone: a sharded run
 *     equals the unsharded one.  A terminated cur counts as R playouts that all
 *     end with its own final board.
 *  3. Back up.  Every node on the path, the root included: v += 1.  Every node
 *     but the root: w += 2 (playouts won by the colour that moved into it) +
 *     (playouts drawn).
 *
 * Outputs (device pointers; visits is required, the others may be NULL; every
 * element of every non-NULL output is written, nothing needs zeroing):
 * visits int32[E][N*N], wins2 int32[E][N*N], best int32[E], tree_nodes
 * int32[E], status uint8[E].  By status (oth_solve's numbers):
 *   DONE        visits[a] / wins2[a] are the v / w of the root's child on
 *               square a, 0 for squares without a child (outside the stored
 *               mask, or not yet made when I < k); best is the root child with
 *               the most visits, then the larger wins2, then the lowest square;
 *               tree_nodes is used.
 *   TERMINATED  meta bit 1 set; NO_MOVE: live, stored possible_moves empty.
 *               visits / wins2 all 0, best -1, tree_nodes 1; nothing is searched.
 *
 * Workspace.  Device memory of at least oth_mcts_workspace_bytes(board_size,
 * n_envs, T) bytes, 8-byte aligned; it needs no initialising and its contents
 * after the call are unspecified (tree reuse between calls is not offered).
 * oth_mcts_workspace_bytes needs no handle and no GPU; OTH_EINVAL for a board
 * size outside [4, 16], n_envs < 1, T outside [N*N, OTH_MCTS_MAX_TREE_NODES] or
 * a NULL bytes.
 *
 * Handle state.  The call reads boards, meta and the stored possible_moves and
 * writes nothing of the handle: boards, meta, possible_moves, the ply counter,
 * the graph offsets and both tallies stay as they are.  It only enqueues work,
 * never synchronises the host and is capturable into a HIP graph; a replay
 * repeats the same search (the graph regions' offsets are not used).  The
 * running time is bounded whatever the input: I iterations of a descent that
 * places a disc per level plus playouts of at most N*N plies.
 *
 * OTH_EINVAL, with nothing launched: NULL params / workspace / visits, a field
 * out of range (these before the handle is looked at), a NULL handle,
 * max_tree_nodes below N*N, workspace_bytes below what
 * oth_mcts_workspace_bytes reports, a misaligned workspace.  Every board size
 * works. */
#define OTH_MCTS_MAX_ITERATIONS 65535
#define OTH_MCTS_MAX_PLAYOUTS   64
#define OTH_MCTS_MAX_C          65535
#define OTH_MCTS_MAX_TREE_NODES (1 << 24)
enum { OTH_MCTS_DONE = 0, OTH_MCTS_TERMINATED = 1, OTH_MCTS_NO_MOVE = 3 };
typedef struct oth_mcts_params {
    int32_t  iterations;      /* I in [1, OTH_MCTS_MAX_ITERATIONS] */
    int32_t  playouts;        /* R in [1, OTH_MCTS_MAX_PLAYOUTS]: random games per evaluated node */
    int32_t  c_explore;       /* C in [0, OTH_MCTS_MAX_C]: exploration constant in 1/256 */
    int32_t  max_tree_nodes;  /* T in [N*N, OTH_MCTS_MAX_TREE_NODES]: node slots per board */
    uint64_t seed;            /* Philox key of the playouts (not the handle's) */
    uint32_t id_key;
    uint64_t counter;         /* < 2^56, as oth_playouts */
} oth_mcts_params;
int oth_mcts_workspace_bytes(int32_t board_size, int32_t n_envs, int32_t max_tree_nodes, uint64_t *bytes);
int oth_mcts(oth_env *env, const oth_mcts_params *p, void *workspace, uint64_t workspace_bytes,
             int32_t *visits, int32_t *wins2, int32_t *best, int32_t *tree_nodes, uint8_t *status,
             oth_stream_t stream);

/* Network-guided tree search per board (no reference counterpart: the rung
 * after oth_mcts, the search of the AlphaZero loop).  Priors steer the
 * selection and a value supplied by the caller replaces the playouts; both are
 * integers, so every output is an exact function of the board, the parameters
 * and the integers supplied, and the mapping to lanes shows in none of them.
 * The evaluation (a policy and value network, say) runs between launches: the
 * tree of a board persists in a workspace the caller supplies, and each
 * oth_puct_advance carries every board's search one simulation further -- it
 * applies the evaluation of the board's pending leaf, descends to the next
 * leaf and emits that leaf as the next input.  E boards give a batch of E
 * leaves a launch; no random number is drawn.
 *
 * Parameters (struct oth_puct_params, host memory, read during the call and
 * baked into the launch; the same values in every call of one search): the
 * exploration constant C in 1/256 and T node slots per board.
 *
 * The tree.  A node holds a position as oth_step with flags 0 leaves it, a
 * pass already resolved, exactly as an oth_mcts node.  It also holds
 *   v  the evaluations backed up through it,
 *   w  an int64: the sum of the backed-up values, counted for the colour that
 *      moved into the node (its parent's side to move),
 *   P  its prior in [0, OTH_PUCT_PRIOR_MAX], its square, and whether its
 *      position has been made (a child exists from its parent's expansion on;
 *      its position is computed when a selection first moves to it).
 * Node 0 is the root and used = 1.
 *
 * oth_puct_begin reads the handle's boards, meta and stored possible_moves and
 * classifies each board as oth_mcts does (oth_solve's status numbers):
 * TERMINATED, NO_MOVE (live, the stored mask empty), otherwise DONE.  A DONE
 * board gets its root, the stored mask (its squares on the board) as the
 * root's move list, and the root is its pending leaf, kind EXPAND (T >= N*N
 * holds the root's children; a stored mask of more than T - 1 squares, which
 * no position of the game has, makes it a VALUE leaf).  Other boards have no
 * pending leaf.  Then the leaves are written (below).
 *
 * oth_puct_advance, for each board with a pending leaf L, s being L's side to
 * move:
 *  1. Value.  Kind TERMINAL: val = OTH_PUCT_VALUE_ONE sign(discs(s) -
 *     discs(other)).  Otherwise val = values[e] clamped to [-OTH_PUCT_VALUE_ONE,
 *     OTH_PUCT_VALUE_ONE]: the value of L for s, in units of 2^-15.
 *  2. Expand, kind EXPAND only (decided at selection time by used + k <= T, k
 *     being L's move count): the slots used .. used+k-1 are reserved for L's
 *     children in ascending square order and used += k.  A child gets its
 *     square, P = priors[e][square] clamped to [0, OTH_PUCT_PRIOR_MAX], v = w =
 *     0, and is not made.  Priors at other squares are never read; kinds VALUE
 *     and TERMINAL read none.
 *  3. Back up.  Every node on the path but the root: v += 1, and w += val if
 *     the colour that moved into it is s, else w -= val.  No other sign logic,
 *     passes included.  The root: v += 1.
 *  4. Select, if more != 0 and the root's v < OTH_PUCT_MAX_SIMS; otherwise the
 *     board has no pending leaf afterwards.  From cur = the root, repeat:
 *       - cur is terminated: stop, kind TERMINAL.
 *       - cur has no reserved children: stop, kind EXPAND if used + k <= T,
 *         else VALUE (the tree is full; cur stays a leaf for the rest of the
 *         search).
 *       - otherwise move to the child c of the largest key, the lowest square
 *         among equal keys,
 *           key = q_c + floor(C P_c isqrt(2^16 v_p) / (2^17 (1 + v_c)))
 *           q_c = 0 if v_c = 0, else floor(w_c / v_c), rounded toward minus
 *                 infinity;
 *         v_p is cur's v (>= 1 whenever cur has children), isqrt the exact
 *         integer floor square root, keys compared as signed 64-bit integers
 *         (the numerator is below 2^52).  q is in units of 2^-15 and the second
 *         term is c P sqrt(v_p) / (1 + v_c) in the same units, c = C / 256 and
 *         P = P_c / 2^16.  If c is not made, its position is made now
 *         (oth_step's ply with flags 0, a pass resolved) and c is the leaf:
 *         stop.
 * A board without a pending leaf ignores priors, values and more.  The call
 * never reads the handle's boards: a search goes on from the root it began
 * with, whatever the handle has done since.
 *
 * Leaves (struct oth_puct_leaves, host memory holding device pointers; the
 * struct or any pointer in it may be NULL; every element of a non-NULL array
 * is written by begin and by advance).  kind uint8[E], boards uint64[E][2W],
 * meta uint16[E], legal uint64[E][W] -- the exchange format of oth_get_state /
 * oth_set_state.  A board with a pending leaf after the call: its kind, and the
 * leaf's position; meta carries the turn, terminated and winner bits as
 * oth_step sets them and no opening plies; legal is the leaf's recomputed move
 * list (none for a terminated leaf, where oth_step on a full board would leave
 * the mask as it was), for the root the stored mask.  A board without one: kind
 * OTH_PUCT_LEAF_NONE and the root with the meta the handle held at begin, so
 * that an evaluator always gets a valid input.  obs (NULL: none), of `layout`
 * and `dtype`, is exactly what oth_observe(layout, dtype) gives for a handle
 * oth_set_state'd to these three arrays, (E, planes, N, N).
 *
 * oth_puct_result may be called at any point of a search and changes nothing.
 * visits int32[E][N*N] is required; value_sums int64[E][N*N], best int32[E],
 * tree_nodes int32[E], status uint8[E] may be NULL; every element of a
 * non-NULL output is written.  DONE boards: visits[a] / value_sums[a] are the
 * v / w of the root's child on square a, 0 elsewhere; best is the child with
 * the most visits, then the larger w, then the lowest square, -1 while no
 * child has a visit (the root unexpanded, or only the root evaluated);
 * tree_nodes is used.  TERMINATED and NO_MOVE boards:
 * zeros, best -1, tree_nodes 1.
 *
 * Workspace.  Device memory of at least oth_puct_workspace_bytes(board_size,
 * n_envs, T) bytes, 8-byte aligned.  It needs no initialising before begin;
 * between the calls of one search it is opaque and must not be moved or
 * written (an advance or result on a workspace that no begin of the same
 * geometry and T wrote does nothing).  One workspace holds one search: it is
 * not oth_mcts' workspace.  oth_puct_workspace_bytes needs no handle and no
 * GPU; OTH_EINVAL as oth_mcts_workspace_bytes.
 *
 * Handle state.  begin reads boards, meta and the stored possible_moves;
 * advance and result read only the handle's geometry.  None of the calls reads
 * or writes the ply counter, the tallies or the graph offsets, and none writes
 * boards, meta or possible_moves.  Each only enqueues work, never synchronises
 * the host and is capturable into a HIP graph; no counter is baked in, so one
 * captured advance replayed S times is S simulations (with the priors and
 * values its pointers hold at each replay).  An advance places at most one disc
 * per level of a path that is at most N*N + 1 levels long: its running time is
 * bounded whatever the input.
 *
 * OTH_EINVAL, with nothing launched: NULL params or workspace, NULL visits
 * (result), NULL priors or values (advance), a field out of range, a
 * misaligned workspace, an unknown layout or dtype beside a non-NULL obs (all
 * these before the handle is looked at), a NULL handle, max_tree_nodes below
 * N*N, workspace_bytes below what oth_puct_workspace_bytes reports.  Every
 * board size works. */
#define OTH_PUCT_VALUE_ONE      32768       /* a certain win, in value units */
#define OTH_PUCT_PRIOR_MAX      65535
#define OTH_PUCT_MAX_C          65535       /* c_puct in 1/256 */
#define OTH_PUCT_MAX_TREE_NODES (1 << 24)
#define OTH_PUCT_MAX_SIMS       ((1 << 24) - 1)
enum { OTH_PUCT_LEAF_NONE = 0, OTH_PUCT_LEAF_EXPAND = 1, OTH_PUCT_LEAF_VALUE = 2, OTH_PUCT_LEAF_TERMINAL = 3 };
typedef struct oth_puct_params {
    int32_t c_puct;          /* C in [0, OTH_PUCT_MAX_C]: exploration constant in 1/256 */
    int32_t max_tree_nodes;  /* T in [N*N, OTH_PUCT_MAX_TREE_NODES]: node slots per board */
} oth_puct_params;
typedef struct oth_puct_leaves {
    uint8_t  *kind;    /* [E] OTH_PUCT_LEAF_* */
    uint64_t *boards;  /* [E][2W] */
    uint16_t *meta;    /* [E] */
    uint64_t *legal;   /* [E][W] */
    void     *obs;     /* (E, planes, N, N) of layout and dtype, as oth_observe */
    int32_t   layout, dtype;
} oth_puct_leaves;
int oth_puct_workspace_bytes(int32_t board_size, int32_t n_envs, int32_t max_tree_nodes, uint64_t *bytes);
int oth_puct_begin(oth_env *env, const oth_puct_params *p, void *workspace, uint64_t workspace_bytes,
                   const oth_puct_leaves *leaves, oth_stream_t stream);
int oth_puct_advance(oth_env *env, const oth_puct_params *p, void *workspace, uint64_t workspace_bytes,
                     const int32_t *priors, const int32_t *values, int32_t more,
                     const oth_puct_leaves *leaves, oth_stream_t stream);
int oth_puct_result(oth_env *env, const oth_puct_params *p, void *workspace, uint64_t workspace_bytes,
                    int32_t *visits, int64_t *value_sums, int32_t *best, int32_t *tree_nodes,
                    uint8_t *status, oth_stream_t stream);

/* Self-play on the search's tree: the move of a search, and the search carried
 * to the position the handle has reached since (the outer loop of AlphaZero-
 * style self-play: advance S times, pick, oth_step, reroot, advance ...).  Both
 * work on oth_puct_begin's workspace, whose size does not change: the re-root
 * works in place.
 *
 * oth_puct_pick changes nothing, like oth_puct_result, and may be called at any
 * point of a search.  actions int32[E] is required; sample uint8[E] may be
 * NULL.  Per board: a status other than DONE gives -1.  Let V be the sum of
 * the root's children's v; V = 0 (the root unexpanded, or only the root
 * evaluated) gives -1.  sample NULL or sample[e] = 0: oth_puct_result's best,
 * exactly.  sample[e] != 0: the move is drawn in proportion to the visits.  u =
 * word 0 of the Philox4x32-10 block of key `seed` and counter words (id,
 * counter lo, counter hi, purpose 4) -- a purpose of its own beside the four
 * of the draws above -- with id = id_key + env_id_base + e mod 2^32; r =
 * floor(u V / 2^32) (the rule for an index among n choices; V < 2^24, the
 * product fits 64 bits); the action is the first child, in ascending squares,
 * whose cumulative v exceeds r.  Any 64-bit counter is accepted, and it is
 * baked into the launch (a captured pick replays the same draw).  The draw
 * depends on the global env id and the counter alone: a sharded run equals the
 * unsharded one.  Temperatures other than 0 and 1 are the caller's business:
 * compute the move from visits and hand its square to oth_puct_reroot.
 *
 * oth_puct_reroot.  The caller has played something on the handle since the
 * search began, normally oth_step(actions).  The call reads the handle's
 * boards, meta and stored possible_moves, as begin does; afterwards the root of
 * every board's search is the handle's position H, with as much of the old tree
 * as still applies.  actions int32[E] is required; root_priors int32[E][N*N]
 * and kept uint8[E] may be NULL.  Per board:
 *  1. Keep test.  All of: the search's status is DONE; the root has reserved
 *     children and actions[e] is the square of one of them, c; H is not
 *     terminated; c's position has H's black discs, white discs and side to
 *     move; c is not terminated; H's stored mask, restricted to the board,
 *     equals c's recomputed move list.  If c was not yet made its position is
 *     made first, exactly as a selection does (oth_step's ply with flags 0, a
 *     pass resolved).  Nothing else is compared: a handle that auto-reset,
 *     played a random-opening ply, took the invalid-move path or was
 *     oth_set_state'd elsewhere simply fails the test.
 *  2. Kept (kept[e] = 1): the subtree of c becomes the tree and c its root.
 *     Every node of the subtree, made or not, keeps its v, w, P, square, made
 *     flag, position and its children in ascending square order; used
 *     (tree_nodes) becomes the number of nodes of the subtree, so the dropped
 *     slots are free for later expansions.  The root's own w is not observable.
 *     Node numbers are opaque: nothing observable depends on them.  The meta
 *     "the handle held at begin" that a NONE leaf shows becomes H's meta.
 *  3. Not kept (kept[e] = 0): exactly what oth_puct_begin does for this board
 *     from H -- status TERMINATED or NO_MOVE, or DONE with a fresh root, used =
 *     1.
 *  4. Root priors.  Where root_priors is not NULL and a kept root has reserved
 *     children, each child's P becomes root_priors[e][square] clamped to [0,
 *     OTH_PUCT_PRIOR_MAX], before the selection of step 5.  Kept roots only: a
 *     fresh root gets its priors at its first advance.  This is how root noise
 *     is applied again: evaluate the stepped handle's position, mix the noise
 *     in (oth_puct_noise in root mode, below), pass the result here.
 *  5. Pending leaf.  Whatever leaf was pending before the call is discarded
 *     (its node stays as it is and can be selected again).  A DONE board whose
 *     root's v < OTH_PUCT_MAX_SIMS runs step 4 of oth_puct_advance from the
 *     root: its pending leaf and kind.  For a fresh or unexpanded root that is
 *     the root itself, kind EXPAND (or VALUE as at begin) -- a kept root that
 *     was a VALUE leaf and now has room included.  Other boards have none.
 *  6. The leaves and obs are written exactly as advance writes them.
 * OTH_EINVAL, with nothing launched: NULL actions, and everything the other
 * oth_puct calls refuse.  The call only enqueues work and is capturable; it
 * writes nothing of the handle; its running time is bounded by used.  Every
 * output is a function of the board's own tree, its handle state and its
 * inputs, never of E, the board's index or the mapping to lanes, and two runs
 * give identical outputs. */
int oth_puct_pick(oth_env *env, const oth_puct_params *p, void *workspace, uint64_t workspace_bytes,
                  const uint8_t *sample, uint64_t seed, uint32_t id_key, uint64_t counter,
                  int32_t *actions, oth_stream_t stream);
int oth_puct_reroot(oth_env *env, const oth_puct_params *p, void *workspace, uint64_t workspace_bytes,
                    const int32_t *actions, const int32_t *root_priors, uint8_t *kept,
                    const oth_puct_leaves *leaves, oth_stream_t stream);

/* Dirichlet root noise for self-play, in integers: oth_puct_noise mixes a keyed
 * draw into the priors of the handle's position, so that a self-play run stays
 * an exact function of the boards, the parameters, the weight bytes and the
 * seeds.  It reads the handle and never writes it, and it knows nothing of a
 * search's workspace: it maps rows of priors to rows of priors.
 *
 * Shapes.  K = rows_per_board in [1, OTH_PUCT_MAX_LEAVES]; priors_in and
 * priors_out are int32[E K][N*N] and may be the same array (otherwise they must
 * not overlap); kind uint8[E K] and boards uint64[E K][2W] are a search's leaf
 * arrays (struct oth_puct_leaves), both given or both NULL; table uint32[4096]
 * is a gamma table on the device (below).
 *
 * Which rows take noise.  The row of board e is row e K; every other row, and
 * the row of a board that is not applied, is copied unchanged (where priors_in
 * == priors_out nothing is written to those rows).  Board e is applied
 *   - in root mode (kind and boards NULL; for oth_puct_reroot's root_priors):
 *     always;
 *   - in leaf mode (for the priors of an advance): where kind[e K] ==
 *     OTH_PUCT_LEAF_EXPAND and the 2W words of boards[e K] equal the handle's
 *     board e, that is, where the pending leaf is the root itself (a deeper
 *     leaf has more discs, so nothing else needs comparing).  In a batch
 *     search a root leaf can only sit in slot 0: the Select takes slot after
 *     slot, a root without children is slot 0's leaf, and any later slot's
 *     descent ends on that same root, which is a collision and closes the board
 *     for the launch; at begin and at a re-root a fresh or unexpanded root is
 *     slot 0's leaf alone.
 *
 * The draw.  Let the legal squares a be those of the handle's stored
 * possible_moves, restricted to the board, in ascending order (noise only ever
 * goes to the handle's position, so the call takes no legal array).  g_a =
 * min(table[u_a >> 20], OTH_NOISE_G_MAX), u_a = word a & 3 of the
 * Philox4x32-10 block of key `seed` and counter words (id, counter lo, counter
 * hi, 6 | (a >> 2) << 8): purpose 6, a purpose of its own, with the block of
 * four squares in bits 8 .. 15 of the purpose word, so that no counter
 * arithmetic of a caller can collide with it; id = id_key + env_id_base + e mod
 * 2^32.  Any 64-bit counter is accepted and is baked into the launch (a
 * captured call replays the same draw); the draw depends on the global env id,
 * the counter and the square alone: a sharded run equals the unsharded one.
 *
 * The mix.  G = the sum of the g_a (at most 2^32).  No legal square, or G = 0:
 * the row is copied.  Otherwise eta_a = floor((65535 g_a + floor(G / 2)) / G)
 * (oth_net_eval's rounding of a prior), and on the legal squares
 *   out_a = ((256 - epsilon) clamp(in_a, 0, 65535) + epsilon eta_a + 128) >> 8,
 * epsilon in [0, 256] in units of 1/256; the other squares of the row are
 * copied.  (epsilon = 0 leaves the clamped inputs.)
 *
 * The table holds 4,096 quantiles of Gamma(alpha, 1), scaled so that the
 * largest is 2^24 - 1: normalised gamma draws are a Dirichlet(alpha) draw, and
 * the normalisation makes the scale free.  The library takes any table; the
 * Python package makes one on the host (dirichlet_table).  A very small alpha
 * gives mostly zero entries, and with them rows that take no noise (G = 0).
 *
 * OTH_EINVAL, with nothing launched: a NULL handle, priors or table; exactly
 * one of kind and boards; rows_per_board outside [1, OTH_PUCT_MAX_LEAVES];
 * epsilon outside [0, 256]; E K not fitting 31 bits.  The call only enqueues
 * work and is capturable. */
#define OTH_NOISE_TABLE 4096      /* entries of a gamma table */
#define OTH_NOISE_G_MAX (1 << 24) /* entries are clamped to this */
int oth_puct_noise(oth_env *env, int32_t rows_per_board, const uint8_t *kind, const uint64_t *boards,
                   const int32_t *priors_in, int32_t *priors_out, int32_t epsilon, const uint32_t *table,
                   uint64_t seed, uint32_t id_key, uint64_t counter, oth_stream_t stream);

/* The batch calls: K leaves a board per launch under virtual loss, so that a
 * network sees E K rows a call and a move of S simulations needs about S / K
 * calls.  Virtual loss only needs an order, and one board's K selections have
 * one by definition -- slot 0, then slot 1, and so on -- so the merge is
 * defined exactly, in integers, like everything above.  The tree, the nodes,
 * the key, steps 1 to 3 of oth_puct_advance and struct oth_puct_leaves are
 * unchanged.
 *
 * Shapes.  A board has K slots, j = 0 .. K-1, K in [1, OTH_PUCT_MAX_LEAVES];
 * row e K + j of every leaf array is slot j of board e: kind uint8[E K], boards
 * uint64[E K][2W], meta uint16[E K], legal uint64[E K][W]; obs (E K, planes, N,
 * N) is exactly oth_observe of a handle of E K boards oth_set_state'd to those
 * three arrays; priors int32[E K][N*N] and values int32[E K] in the same rows.
 * Every element of every non-NULL array is written by each of the three calls.
 * A slot without a leaf is written as a board without one is written by the
 * plain calls: kind OTH_PUCT_LEAF_NONE and the root, with the meta the handle
 * held at begin or at the last re-root.  E K must fit 31 bits.
 *
 * oth_puct_begin_batch is oth_puct_begin: a DONE board's root is the leaf of
 * slot 0 (EXPAND, or VALUE as there); slots 1 .. K-1 are NONE.
 *
 * oth_puct_advance_batch, per board:
 *  1. Apply.  For j = 0 .. K-1 in ascending order, each slot with a leaf runs
 *     steps 1 to 3 of oth_puct_advance with that row's priors and value: the
 *     value, the expansion for kind EXPAND, the backup.  Expansions therefore
 *     take their child blocks in slot order.  Afterwards no slot holds a leaf.
 *  2. Select.  sim_limit is in [0, OTH_PUCT_MAX_SIMS]; 0 selects nothing (more
 *     = 0).  Let r = used (the slots reserved so far) and n_x = 0 for every
 *     node x (the paths of this launch through x).  For j = 0 .. K-1:
 *       - the board is closed (below), or the root's v + j >= sim_limit: slot j
 *         is NONE.
 *       - otherwise descend from the root exactly as step 4 of oth_puct_advance
 *         does, with every statistic read through the launch's virtual loss:
 *           v'_c = v_c + n_c,  w'_c = w_c - OTH_PUCT_VALUE_ONE n_c,
 *           v'_p = v_p + n_p,
 *           key = q'_c + floor(C P_c isqrt(2^16 v'_p) / (2^17 (1 + v'_c))),
 *           q'_c = 0 if v'_c = 0, else floor(w'_c / v'_c) toward minus infinity.
 *         There is no sign logic: w is already counted for the side that
 *         chooses among the siblings, and a path in flight is one loss for it.
 *         The bounds of the plain key hold: v' < 2^24 because of sim_limit,
 *         |w'| <= 2^15 v', and the numerator stays below 2^52.
 *       - the descent stops as there: at a terminated node, at a node without
 *         reserved children, or at a child that is not yet made, which is made
 *         now.  Let X be the node where it stops.
 *           X terminated: kind TERMINAL.  Several slots of one launch may hold
 *             the same terminated node; each is a simulation of its own and no
 *             evaluation is spent on it.
 *           X is already the leaf of an earlier slot of this launch (a
 *             collision): the board is closed for this launch, slot j and all
 *             later slots are NONE, and path j counts nowhere.
 *           otherwise, k being X's move count: if r + k <= T, kind EXPAND and
 *             r += k; else kind VALUE.  Reservations of earlier slots count, so
 *             every EXPAND leaf still fits when step 1 of the next launch
 *             applies them in slot order.
 *       - where slot j got a leaf, n_x += 1 for every node x on its path, the
 *         root included.
 *  3. Virtual loss does not survive the launch: when the call returns every
 *     node holds its real v and w only, and oth_puct_result, oth_puct_pick and
 *     the re-root's keep test and compaction see the tree the backups made.
 * A board all of whose slots are NONE ignores priors, values and sim_limit.
 * A search of S simulations passes sim_limit = S in every call and launches
 * until no slot holds a leaf: every DONE board then has exactly S, however its
 * batches closed.
 *
 * K = 1.  No virtual loss is ever read and no collision can occur: the call is
 * oth_puct_advance with more = (the root's v after the backup < sim_limit),
 * byte for byte in every output -- more = 0 for sim_limit = 0, more = 1 for
 * sim_limit = OTH_PUCT_MAX_SIMS.  begin_batch is oth_puct_begin, and
 * reroot_batch is oth_puct_reroot on every board whose new root's v is below
 * sim_limit (on every board for sim_limit = OTH_PUCT_MAX_SIMS).
 *
 * oth_puct_reroot_batch is oth_puct_reroot with steps 1 to 4 and 6 unchanged.
 * Step 5: every slot's leaf is discarded, and a DONE board runs the Select
 * above from the new root with sim_limit.  A fresh or unexpanded root is the
 * leaf of slot 0 alone (slot 1 collides with it).
 *
 * Workspace.  At least oth_puct_batch_workspace_bytes(board_size, n_envs, T, K)
 * bytes, which is never less than oth_puct_workspace_bytes reports, 8-byte
 * aligned, opaque; it holds one search.  oth_puct_result and oth_puct_pick work
 * on it unchanged (same handle geometry and T).  A search goes on with the
 * family that began it: a batch call on a workspace that no begin_batch of the
 * same geometry, T and K wrote does nothing; a plain advance or reroot on a
 * batch workspace stays inside the workspace's memory, and what the search does
 * afterwards is unspecified.  oth_puct_batch_workspace_bytes needs no handle
 * and no GPU; OTH_EINVAL where oth_puct_workspace_bytes gives it, and for K
 * outside [1, OTH_PUCT_MAX_LEAVES].
 *
 * Handle state, capture and determinism: as the plain calls.  begin_batch and
 * reroot_batch read boards, meta and the stored possible_moves, advance_batch
 * only the geometry; none writes anything of the handle.  Each only enqueues
 * work, is capturable and draws no random number.  Every output is a function
 * of the board's tree, K, sim_limit and that board's K rows of integers alone,
 * never of E, the board's index or the mapping to lanes.  The running time is
 * bounded by K descents of at most N*N + 1 levels (and the re-root's by used).
 *
 * OTH_EINVAL, with nothing launched: everything the plain calls refuse, K or
 * sim_limit out of range (before the handle is looked at), E K above 2^31 - 1,
 * workspace_bytes below what oth_puct_batch_workspace_bytes reports. */
#define OTH_PUCT_MAX_LEAVES 64
int oth_puct_batch_workspace_bytes(int32_t board_size, int32_t n_envs, int32_t max_tree_nodes, int32_t K,
                                   uint64_t *bytes);
int oth_puct_begin_batch(oth_env *env, const oth_puct_params *p, int32_t K, void *workspace,
                         uint64_t workspace_bytes, const oth_puct_leaves *leaves, oth_stream_t stream);
int oth_puct_advance_batch(oth_env *env, const oth_puct_params *p, int32_t K, void *workspace,
                           uint64_t workspace_bytes, const int32_t *priors, const int32_t *values,
                           int32_t sim_limit, const oth_puct_leaves *leaves, oth_stream_t stream);
int oth_puct_reroot_batch(oth_env *env, const oth_puct_params *p, int32_t K, void *workspace,
                          uint64_t workspace_bytes, const int32_t *actions, const int32_t *root_priors,
                          uint8_t *kept, int32_t sim_limit, const oth_puct_leaves *leaves,
                          oth_stream_t stream);

/* The replay store: the self-play samples kept, labelled and drawn on the
 * device (no reference counterpart: the training side of the AlphaZero loop).
 * A learner trains on the triple (position, visit target, outcome from the
 * mover's side), drawn as random minibatches under the eight symmetries of the
 * board.  The store keeps, for each of the E boards of a handle geometry, a
 * ring of H record slots in a workspace the caller supplies; every output is
 * an exact integer function of the inputs, and the mapping to lanes shows in
 * none of them.
 *
 * Geometry and workspace.  Every call names the store's geometry: the
 * handle's (N, E), `horizon` H in [1, OTH_REPLAY_MAX_HORIZON] with E H <=
 * OTH_REPLAY_MAX_ROWS, and `max_batch` B in [1, OTH_REPLAY_MAX_BATCH], the
 * most rows one gather or sample writes.  The workspace is device memory of at
 * least oth_replay_workspace_bytes(board_size, n_envs, H, B) bytes, 8-byte
 * aligned and opaque.  It needs no initialising before oth_replay_begin and
 * holds no addresses, so a byte copy of it is a checkpoint of the store.
 * Every other replay call on a workspace that no oth_replay_begin of the same
 * geometry (N, E, H, B) wrote does nothing.  oth_replay_workspace_bytes needs
 * no handle and no GPU; OTH_EINVAL as oth_puct_workspace_bytes gives it, and
 * for H, B or E H out of range.
 *
 * Row e H + j is slot j of board e.  A row holds a state (OTH_REPLAY_EMPTY,
 * _OPEN or _LABELLED), black[W], white[W], legal[W], the turn bit, visits
 * int32[N*N] and an outcome int32.  Per board the store also keeps count (the
 * records made; count mod H is the next slot), span in [0, H] (the current
 * game's records still in the ring) and last_turn.
 *
 * oth_replay_begin.  Every row becomes EMPTY, count and span become 0.  The
 * call reads only the handle's geometry.
 *
 * oth_replay_append.  visits int32[E][N*N] is required; skip uint8[E] may be
 * NULL.  The call reads the handle's boards, meta and stored possible_moves
 * and writes nothing of the handle.  Per board, last_turn = meta bit 0,
 * always.  The cleaned visits are c[a] = clamp(visits[a], 0, 2^24 - 1) where a
 * is in the stored mask (restricted to the board), else 0.  The board records
 * iff it is not terminated, skip is NULL or skip[e] = 0, and the sum of c is
 * positive.  Recording: slot j = count mod H is overwritten, whatever its
 * state; the row takes the discs, the stored mask, the turn bit and c; its
 * state becomes OPEN and its outcome 0; count += 1; span = min(span + 1, H).
 * A board that does not record changes nothing but last_turn.  A game with
 * more than H records loses its oldest OPEN rows to its newest.
 *
 * oth_replay_label.  rewards int32[E] and dones uint8[E] are required; the
 * call reads only the geometry.  Per board with dones[e] != 0: z =
 * clamp(rewards[e], -32768, 32768); every OPEN row among the board's last span
 * records becomes LABELLED with outcome +z if the row's turn bit equals
 * last_turn, else -z; span becomes 0.  Boards with dones[e] = 0 are untouched.
 * The caller's side of the contract: rewards[e] is the result for the side
 * that was to move at the board's latest append -- exactly what oth_step
 * reports for the ply played from that position, with and without
 * OTH_DISK_REWARD, on the sudden-death path and with OTH_AUTO_RESET (the
 * handle is not read); oth_step_vs' reward is the protagonist's, who is that
 * side too.
 *
 * oth_replay_counts.  out, device int64[3]: the rows in state EMPTY, OPEN and
 * LABELLED.
 *
 * Batches (struct oth_replay_batch, host memory holding device pointers; any
 * pointer may be NULL; every element of every non-NULL array is written), n
 * rows: state uint8[n], boards uint64[n][2W], meta uint16[n], legal
 * uint64[n][W], visits int32[n][N*N], outcome int32[n], obs of `layout` and
 * `dtype`, rows int32[n], sym uint8[n].
 *
 * Symmetry s in [0, 8).  For stored square a = (r, c): (r1, c1) = (c, r) if
 * s & 1, else (r, c); r2 = N - 1 - r1 if s & 2, else r1; c2 = N - 1 - c1 if
 * s & 4, else c1; sigma_s(a) = r2 N + c2: the eight elements of the square's
 * symmetry group.  Row i of a batch built from store row rho under s: bit
 * sigma_s(a) of black, white and legal is bit a of the stored words (squares
 * off the board are dropped); visits[sigma_s(a)] is the stored visits[a]; meta
 * is the turn bit alone (no terminated bit, no winner, no opening plies);
 * outcome and state are as stored; obs is exactly what oth_observe(layout,
 * dtype) gives for a handle of n boards oth_set_state'd to those three arrays,
 * (n, planes, N, N).  An EMPTY row gives zeros everywhere, with state 0.
 *
 * oth_replay_gather.  rows_in int32[n] (required) and sym_in uint8[n] (NULL:
 * all 0) are device inputs, n in [1, B].  Row i is store row rows_in[i] under
 * sym_in[i] & 7; a row number outside [0, E H) gives the EMPTY row.
 * batch->rows and batch->sym echo what was used, with -1 for an out-of-range
 * row.  This is the dump the tests read the store through, and how a caller
 * with priorities of its own draws.
 *
 * oth_replay_sample.  M being the number of LABELLED rows, for i in [0, n):
 * (u0, u1) are words 0 and 1 of the Philox4x32-10 block of key `seed` and
 * counter words (id_key + i mod 2^32, counter lo, counter hi, purpose 5) -- a
 * purpose of its own beside the five of the draws above; r = floor(u0 M /
 * 2^32); the row is the (r + 1)-th LABELLED row in ascending row number; s =
 * u1 >> 29 if augment != 0, else 0; then as gather.  M = 0 gives every row
 * EMPTY and rows -1.  Any 64-bit counter is accepted and is baked into the
 * launch (a captured sample replays the same draw on whatever the store then
 * holds).  The draw depends on this store alone, not on env_id_base: a sharded
 * run does not repeat an unsharded one.
 *
 * oth_symmetry_masks is stateless, like oth_legal_moves: in and out are device
 * uint64[n][planes][W], sym uint8[n]; every plane of row i is transformed by
 * sym[i] & 7.  in == out is OTH_EINVAL.
 *
 * Handle state and capture.  Only append reads the handle's boards; none of
 * the calls writes anything of the handle.  Each only enqueues work, never
 * synchronises the host and is capturable into a HIP graph.  append and label
 * bake nothing in, so a captured self-play move replays correctly.
 *
 * OTH_EINVAL, with nothing launched: NULL required pointers (workspace,
 * visits, rewards, dones, out, batch, rows_in; sym, in, out of
 * oth_symmetry_masks), n, H or B out of range, a misaligned workspace, an
 * unknown layout or dtype beside a non-NULL obs (all these before the handle is
 * looked at), a NULL handle, E H above OTH_REPLAY_MAX_ROWS, workspace_bytes
 * below what oth_replay_workspace_bytes reports, n above B.  Every board size
 * works. */
#define OTH_REPLAY_MAX_HORIZON 65536
#define OTH_REPLAY_MAX_ROWS    (1 << 24)
#define OTH_REPLAY_MAX_BATCH   (1 << 20)
enum { OTH_REPLAY_EMPTY = 0, OTH_REPLAY_OPEN = 1, OTH_REPLAY_LABELLED = 2 };
typedef struct oth_replay_batch {
    uint8_t  *state;    /* [n] OTH_REPLAY_* */
    uint64_t *boards;   /* [n][2W] */
    uint16_t *meta;     /* [n] */
    uint64_t *legal;    /* [n][W] */
    int32_t  *visits;   /* [n][N*N] */
    int32_t  *outcome;  /* [n] */
    void     *obs;      /* (n, planes, N, N) of layout and dtype, as oth_observe */
    int32_t   layout, dtype;
    int32_t  *rows;     /* [n] the store row used, -1: none */
    uint8_t  *sym;      /* [n] the symmetry used */
} oth_replay_batch;
int oth_replay_workspace_bytes(int32_t board_size, int32_t n_envs, int32_t horizon, int32_t max_batch,
                               uint64_t *bytes);
int oth_replay_begin(oth_env *env, int32_t horizon, int32_t max_batch, void *workspace, uint64_t workspace_bytes,
                     oth_stream_t stream);
int oth_replay_append(oth_env *env, int32_t horizon, int32_t max_batch, void *workspace, uint64_t workspace_bytes,
                      const int32_t *visits, const uint8_t *skip, oth_stream_t stream);
int oth_replay_label(oth_env *env, int32_t horizon, int32_t max_batch, void *workspace, uint64_t workspace_bytes,
                     const int32_t *rewards, const uint8_t *dones, oth_stream_t stream);
int oth_replay_counts(oth_env *env, int32_t horizon, int32_t max_batch, void *workspace, uint64_t workspace_bytes,
                      int64_t *out, oth_stream_t stream);
int oth_replay_gather(oth_env *env, int32_t horizon, int32_t max_batch, void *workspace, uint64_t workspace_bytes,
                      int32_t n, const int32_t *rows_in, const uint8_t *sym_in, const oth_replay_batch *batch,
                      oth_stream_t stream);
int oth_replay_sample(oth_env *env, int32_t horizon, int32_t max_batch, void *workspace, uint64_t workspace_bytes,
                      int32_t n, int32_t augment, uint64_t seed, uint32_t id_key, uint64_t counter,
                      const oth_replay_batch *batch, oth_stream_t stream);
int oth_symmetry_masks(int32_t board_size, int32_t n, int32_t planes, const uint8_t *sym, const uint64_t *in,
                       uint64_t *out, oth_stream_t stream);

/* The network: an int8 policy-value MLP evaluated on rows in the exchange
 * format, one launch for any number of rows (no reference counterpart: the
 * evaluator of the AlphaZero loop).  Its outputs are exactly the `priors` and
 * `values` that oth_puct_advance and oth_puct_advance_batch take, and every one
 * of them is an exact integer function of the row, the parameters and the weight
 * bytes: no float is involved.  The calls are stateless and take no handle.
 *
 * Geometry.  N is the board size, nn = N N, W the words of a board.  There are
 * F = 3 nn input features, L hidden layers (1 <= L <= OTH_NET_MAX_LAYERS), all of
 * one width H, a multiple of 64 in [64, OTH_NET_MAX_WIDTH], and a head of nn + 1
 * rows: nn policy rows and one value row.
 *
 * Parameters (struct oth_net_params, host memory read during the call, named in
 * every call): layers = L, width = H, shift[l] for layer l < L (the others are
 * not read), policy_shift and value_shift; every shift read is in [0, 24].
 *
 * Logical weights (oth_net_pack's host inputs).  w: int8, w[0] [H][F], then
 * w[l] [H][H] for 1 <= l < L, then the head wh [nn + 1][H], one after the other.
 * b: int32, b[l] [H] for l < L, then bh [nn + 1].  Every bias satisfies |b| <=
 * 2^30 = OTH_NET_BIAS_MAX.  With that bound no accumulator leaves int32: the
 * first layer is at most 768 * 128 + 2^30 in magnitude (768 = 3 * 256 features of
 * 0 or 1), every later layer and the head at most 512 * 127 * 128 + 2^30 (512
 * inputs in [0, 127]).
 *
 * One row is boards uint64[2W] (black words, then white), meta uint16 and legal
 * uint64[W].  The mover's words are the white words if meta bit 0 is set, else
 * the black words; the other colour's are the opponent's.  For a < nn: x[a] is
 * the mover's bit a, x[nn + a] the opponent's bit a, x[2 nn + a] bit a of legal.
 * Bits at or above nn and every other meta bit are never read; the kind of a
 * leaf is not an input.
 *   h_0 = x.  For l < L: acc = b[l][j] + sum_i w[l][j][i] h_l[i], and
 *   h_{l+1}[j] = min(127, max(0, acc >> shift[l])), an arithmetic shift.
 *   z[o] = bh[o] + sum_j wh[o][j] h_L[j], o = 0 .. nn.
 *   value = clamp(z[nn] >> value_shift, -32768, 32768).
 *
 * Priors.  M is the set of squares a < nn whose legal bit is set.  If M is
 * empty every prior is 0.  Otherwise m = max over M of z[a]; d = (m - z[a]) >>
 * policy_shift with the difference taken in 64 bits; i = d >> 8, f = d & 255;
 * e_a = 0 if i >= 31, else EXP2[f] >> i; S = sum over M of e_a, an int64 (S >=
 * 2^30: the maximum contributes EXP2[0]); prior[a] = floor((65535 e_a + floor(S
 * / 2)) / S) for a in M and 0 outside M.  EXP2[f] = round(2^30 2^(-f / 256)), the
 * 256 literal constants of csrc/net.hpp (EXP2[0] = 1073741824, EXP2[1] =
 * 1070838486, EXP2[255] = 538326517; no entry is nearer than 0.0054 to a
 * rounding tie).  This is round(65535 softmax over the legal squares) with
 * logits in units of 2^-(8 + policy_shift) octaves; the value is in units of
 * 2^-15 = 1 / OTH_PUCT_VALUE_ONE.
 *
 * oth_net_blob_bytes: the size of the packed weights.  Needs no GPU.
 * oth_net_pack: host memory to host memory; validates every range above and
 * writes the device layout of the weights into blob (blob_bytes at least what
 * oth_net_blob_bytes reports, blob 16-byte aligned).  The layout is the library's
 * and opaque; it holds no addresses, so a byte copy to the device is all that is
 * needed, and it depends on (board_size, params): an evaluation that names
 * another geometry or other shifts than the blob was packed for writes nothing.
 * oth_net_eval: boards uint64[R][2W], meta uint16[R], legal uint64[R][W] and blob
 * are device inputs, R = n_rows in [0, OTH_NET_MAX_ROWS]; priors int32[R][nn] and
 * values int32[R] are written; logits int32[R][nn + 1] (z, for tests) may be
 * NULL.  Rows are independent of each other and of how they are batched.  The
 * call only enqueues work (one launch; none for R = 0), never synchronises and
 * is capturable into a HIP graph.
 *
 * OTH_EINVAL, with nothing launched or written: NULL pointers (all but logits), a
 * board size, a field of params or a bias out of range, blob_bytes below what
 * oth_net_blob_bytes reports, a blob that is not 16-byte aligned, n_rows outside
 * [0, OTH_NET_MAX_ROWS]. */
#define OTH_NET_MAX_LAYERS 4
#define OTH_NET_MAX_WIDTH  512
#define OTH_NET_MAX_SHIFT  24
#define OTH_NET_BIAS_MAX   (1 << 30)
#define OTH_NET_MAX_ROWS   (1 << 24)
typedef struct oth_net_params {
    int32_t layers;       /* L in [1, 4] */
    int32_t width;        /* H: a multiple of 64 in [64, 512] */
    int32_t shift[4];     /* shift[l], l < L, in [0, 24] */
    int32_t policy_shift; /* in [0, 24] */
    int32_t value_shift;  /* in [0, 24] */
} oth_net_params;
int oth_net_blob_bytes(int32_t board_size, const oth_net_params *params, uint64_t *bytes);
int oth_net_pack(int32_t board_size, const oth_net_params *params, const int8_t *w, const int32_t *b, void *blob,
                 uint64_t blob_bytes);
int oth_net_eval(int32_t board_size, int32_t n_rows, const oth_net_params *params, const void *blob,
                 uint64_t blob_bytes, const uint64_t *boards, const uint16_t *meta, const uint64_t *legal,
                 int32_t *priors, int32_t *values, int32_t *logits, oth_stream_t stream);

/* The n-tuple network: a sum of look-up tables indexed by the contents of small
 * sets of squares, applied under the eight board symmetries and trained by a
 * delta rule (no reference counterpart: the learned evaluation of the
 * Othello-learning literature, where oth_search's weighted piece counter is
 * the hand-made one).  It evaluates rows in the exchange format, learns from
 * them, and sits at the frontier of the alpha-beta search.  Everything is an
 * exact integer function of its inputs; the training step is a scatter-add of
 * integers and so does not depend on any order.
 *
 * Geometry.  N is the board size, nn = N N, W the words of a board, sigma_s
 * (s in [0, 8)) the symmetry defined for oth_replay_gather above.
 *
 * Parameters (struct oth_ntuple_params, host memory read during the call, named
 * in every call): tuples = T in [1, OTH_NTUPLE_MAX_TUPLES]; length[t] = l_t in
 * [1, OTH_NTUPLE_MAX_LENGTH] for t < T; squares[t][i] = q_{t,i} in [0, nn) for
 * i < l_t, distinct within a tuple; value_shift in [0, 24].  Fields beyond T or
 * l_t are not read.
 *
 * Weights.  A device array int32[n_weights + 1], n_weights = sum_t 3^l_t.  Tuple
 * t's table starts at off_t = sum_{u < t} 3^l_u; the last element is the bias.
 * They are a plain array, part of no packed blob: the learner owns them.
 *
 * One row is boards uint64[2W] (black words, then white) and meta uint16; the
 * mover's words M are the white words if meta bit 0 is set, else the black
 * words, the other colour's are O.  Every other meta bit and bits at or above
 * nn are never read.
 *   cell code  c(a) = 1 if a in M, else 2 if a in O, else 0 (M wins on a square
 *              set in both: no index leaves its table on an unreachable row).
 *   index      idx_{t,s} = sum_{i < l_t} 3^i c(sigma_s(q_{t,i})).
 *   sum        S = bias + sum_t sum_{s < 8} w[off_t + idx_{t,s}], an int64.  A
 *              tuple that a symmetry maps onto itself hits one entry more than
 *              once, and every hit counts.
 *   value      clamp(S >> value_shift, -32768, 32768), an arithmetic shift: from
 *              the mover's side, in units of 1 / OTH_PUCT_VALUE_ONE -- what
 *              oth_puct_advance takes as `values`.
 *
 * oth_ntuple_weight_count: n_weights + 1.  Needs no GPU.
 * oth_ntuple_plan_bytes, oth_ntuple_plan: host memory to host memory, like
 * oth_net_pack; they validate every range above.  The plan holds the 8 T
 * transformed square lists, the offsets and a header that identifies
 * (board_size, params); it is the library's, opaque, and holds no addresses, so
 * a byte copy to the device is all that is needed (plan 8-byte aligned, there
 * and here).  A call that names another geometry or other parameters than the
 * plan was made for writes nothing.
 *
 * oth_ntuple_eval.  boards uint64[R][2W], meta uint16[R], plan and weights are
 * device inputs, R = n_rows in [0, OTH_NTUPLE_MAX_ROWS]; values int32[R] is
 * written; sums int64[R] (S) may be NULL.  Rows are independent of each other
 * and of how they are batched.  One launch (none for R = 0); the call keeps no
 * state, never synchronises and is capturable into a HIP graph.
 *
 * oth_ntuple_update: one delta-rule step on the R rows, with batch semantics.
 * With v_r the value of row r under the weights as they are before the call,
 *   d_r = clamp(round((clamp(targets[r], -32768, 32768) - v_r) rate),
 *               -2^30, 2^30),
 * round(x) = (x + 2^(rate_shift - 1)) >> rate_shift in int64 for rate_shift >=
 * 1 and x for rate_shift 0; rate in [0, OTH_NTUPLE_MAX_RATE], rate_shift in [0,
 * OTH_NTUPLE_MAX_RATE_SHIFT].  (Round to nearest, not a truncating shift: that
 * one gives 0 for small positive errors and -1 for small negative ones, and the
 * weights drift.)  Afterwards every one of the 8 T entries a row hits has had
 * d_r added once per hit, and the bias once; sums over rows are taken modulo
 * 2^32 in two's complement.  deltas int32[R] (d_r) is required and written.
 * Two launches in stream order: the first computes every d_r from the old
 * weights, the second adds with device-scope relaxed atomics on uint32.
 * Integer addition commutes: the weights afterwards do not depend on the order
 * of arrival or the mapping.  targets int32[R] is a device input.
 *
 * oth_search_ntuple: oth_search's contract word for word -- rules, statuses,
 * nodes, the root's stored possible_moves, determinism, outputs -- but for rule
 * 2: the frontier's H(M, O) is the value above of the row (M to move against
 * O).  |value| <= 2^15 and |T| <= 32767 * 256 < 2^23 keep every value strictly
 * inside (-2^24, 2^24).  H is not antisymmetric in general: it is taken from the
 * side to move at the frontier, whoever placed the last disc.
 *
 * OTH_EINVAL, with nothing launched or written: NULL required pointers, a
 * board size or a field of params out of range, plan_bytes below what
 * oth_ntuple_plan_bytes reports, a plan that is not 8-byte aligned,
 * weight_count below what oth_ntuple_weight_count reports, n_rows, rate,
 * rate_shift, depth, terminal_weight or max_nodes out of range (the search's
 * as oth_search's).  Every board size works. */
#define OTH_NTUPLE_MAX_TUPLES     32
#define OTH_NTUPLE_MAX_LENGTH     8
#define OTH_NTUPLE_MAX_ROWS       (1 << 24)
#define OTH_NTUPLE_MAX_RATE       (1 << 24)
#define OTH_NTUPLE_MAX_RATE_SHIFT 40
typedef struct oth_ntuple_params {
    int32_t tuples;          /* T in [1, 32] */
    int32_t length[32];      /* l_t in [1, 8], t < T */
    int32_t squares[32][8];  /* q_{t,i} in [0, N*N), i < l_t, distinct within a tuple */
    int32_t value_shift;     /* in [0, 24] */
} oth_ntuple_params;
int oth_ntuple_weight_count(int32_t board_size, const oth_ntuple_params *params, uint64_t *count);
int oth_ntuple_plan_bytes(int32_t board_size, const oth_ntuple_params *params, uint64_t *bytes);
int oth_ntuple_plan(int32_t board_size, const oth_ntuple_params *params, void *plan, uint64_t plan_bytes);
int oth_ntuple_eval(int32_t board_size, int32_t n_rows, const oth_ntuple_params *params, const void *plan,
                    uint64_t plan_bytes, const int32_t *weights, uint64_t weight_count, const uint64_t *boards,
                    const uint16_t *meta, int32_t *values, int64_t *sums, oth_stream_t stream);
int oth_ntuple_update(int32_t board_size, int32_t n_rows, const oth_ntuple_params *params, const void *plan,
                      uint64_t plan_bytes, int32_t *weights, uint64_t weight_count, const uint64_t *boards,
                      const uint16_t *meta, const int32_t *targets, int32_t rate, int32_t rate_shift, int32_t *deltas,
                      oth_stream_t stream);
int oth_search_ntuple(oth_env *env, int32_t depth, const oth_ntuple_params *params, const void *plan,
                      uint64_t plan_bytes, const int32_t *weights, uint64_t weight_count, int32_t terminal_weight,
                      uint64_t max_nodes, int32_t *value, int32_t *best, int32_t *move_values, uint8_t *status,
                      uint64_t *nodes, oth_stream_t stream);

/* The convolutional network: an int8 residual 3 x 3 convolutional policy-value
 * network on the same rows, with the same outputs and under the same contract as
 * oth_net_* above: every output is an exact integer function of the row, the
 * parameters and the weight bytes; the calls are stateless and take no handle.
 *
 * Geometry.  N is the board size, nn = N N, square a = row N + col.  C =
 * channels is 64 or 128, B = blocks in [1, OTH_CNET_MAX_BLOCKS].  Parameters
 * (struct oth_cnet_params, host memory read during the call): channels, blocks,
 * shift_stem, shift[l] for l < 2 B (the others are not read), shift_head,
 * policy_shift, value_shift; every shift read is in [0, OTH_NET_MAX_SHIFT].
 *
 * conv(w, b, in)[o][y][x] = b[o] + sum_i sum_{dy, dx in {-1, 0, 1}}
 *   w[o][i][dy + 1][dx + 1] in[i][y + dy][x + dx], with in = 0 off the board.
 * clip(v) = min(127, max(0, v)); >> is the arithmetic shift.
 *
 * The input is three planes of 0 or 1 over the squares: the mover's discs (the
 * white words where meta bit 0 is set, else the black words), the opponent's,
 * and the legal squares.  Bits at or above nn and every other meta bit are
 * never read.
 *   stem:     h = clip(conv(3 -> C) >> shift_stem)
 *   block k:  t = clip(conv_2k(h) >> shift[2k]),
 *             h = clip((conv_2k+1(t) >> shift[2k+1]) + h)       k = 0 .. B - 1
 *   head:     one conv C -> 16 with accumulators u[j][a]; the logit of square a is
 *             z[a] = u[0][a], the raw accumulator; f[j][a] = clip(u[j][a] >>
 *             shift_head) for j = 1 .. 15; z[nn] = bv + sum_a sum_{j = 1 .. 15}
 *             wv[a][j - 1] f[j][a]; value = clamp(z[nn] >> value_shift, -32768,
 *             32768).
 * Priors: oth_net's integer softmax (above) over the legal squares from z[a],
 * with EXP2 and policy_shift as there; a row without a legal square gets
 * all-zero priors.
 *
 * No accumulator leaves int32: every bias satisfies |b| <= 2^30 =
 * OTH_NET_BIAS_MAX; a conv's sum is at most 9 * 128 * 127 * 128 < 2^25 in
 * magnitude beside it, the value's sum at most 15 * 256 * 127 * 128 < 2^26.
 *
 * Logical weights (oth_cnet_pack's host inputs), one after the other.  w: int8,
 * the stem [C][3][3][3] as (o, i, ky, kx), the 2 B convs [C][C][3][3], the head
 * [16][C][3][3], then wv [nn][15].  b: int32, the stem's C, the convs' 2 B C,
 * the head's 16, then bv.
 *
 * oth_cnet_blob_bytes, oth_cnet_pack and oth_cnet_eval take what their oth_net_*
 * namesakes take and fail as they do (OTH_EINVAL with nothing launched or
 * written: NULL pointers (all but logits), a board size, a field of params or a
 * bias out of range, blob_bytes below what oth_cnet_blob_bytes reports, a blob
 * that is not 16-byte aligned, n_rows outside [0, OTH_NET_MAX_ROWS]).  The blob
 * is opaque, holds no addresses and begins with two tags (geometry, shifts)
 * whose prefixes differ from oth_net's; an evaluation that names another
 * geometry or other shifts than the blob was packed for writes nothing.
 * oth_cnet_eval is one launch (none for n_rows = 0), never synchronises and is
 * capturable; logits int32[R][nn + 1] (z) may be NULL. */
#define OTH_CNET_MAX_BLOCKS 8
typedef struct oth_cnet_params {
    int32_t channels;     /* C: 64 or 128 */
    int32_t blocks;       /* B in [1, 8] */
    int32_t shift_stem;   /* in [0, 24] */
    int32_t shift[16];    /* shift[l], l < 2 B, in [0, 24] */
    int32_t shift_head;   /* in [0, 24] */
    int32_t policy_shift; /* in [0, 24] */
    int32_t value_shift;  /* in [0, 24] */
} oth_cnet_params;
int oth_cnet_blob_bytes(int32_t board_size, const oth_cnet_params *params, uint64_t *bytes);
int oth_cnet_pack(int32_t board_size, const oth_cnet_params *params, const int8_t *w, const int32_t *b, void *blob,
                  uint64_t blob_bytes);
int oth_cnet_eval(int32_t board_size, int32_t n_rows, const oth_cnet_params *params, const void *blob,
                  uint64_t blob_bytes, const uint64_t *boards, const uint16_t *meta, const uint64_t *legal,
                  int32_t *priors, int32_t *values, int32_t *logits, oth_stream_t stream);

/* OthelloEnv (othello.py:96-214) for every env: the protagonist's colour per
 * env (protagonist: device int8[E] of +1 white / -1 black, NULL = all white,
 * the reference default) and an embedded opponent played on the device
 * (OTH_POLICY_RANDOM / OTH_POLICY_GREEDY).
 *   oth_reset_vs: OthelloEnv.reset (:151-174) -- reset, then the opponent
 *     replies (with its policy) until the protagonist is to move.
 *   oth_step_vs:  OthelloEnv.step (:176-200) -- the protagonist plays
 *     actions[e] (a random move while random-opening plies remain), then the
 *     opponent replies until the protagonist is to move again or the game
 *     ends.  rewards[e] is the protagonist's step reward, negated when an
 *     opponent ply ended the game (:200); plies[e] (may be NULL) counts the
 *     plies applied.  With OTH_AUTO_RESET a finished env is reset_vs'd.
 * Random draws: the j-th ply of call number c (the handle's ply counter,
 * advanced by one per call) uses Philox block (c*256 + j) / 4, word (c*256 + j) % 4. */
int oth_reset_vs(oth_env *env, int32_t opponent_policy, const int8_t *protagonist, const uint8_t *mask,
                 oth_stream_t stream);
int oth_step_vs(oth_env *env, int32_t opponent_policy, const int32_t *actions, const int8_t *protagonist,
                int32_t *rewards, uint8_t *dones, int32_t *plies, oth_stream_t stream);
/* oth_step_vs, then the observation (layout / dtype as oth_observe) of the
 * boards as the call leaves them -- OthelloEnv.step's returned obs
 * (othello.py:200) with OTH_OBS_BOARD -- into obs in the same call: one launch
 * for one-word boards against a random or greedy opponent with obs aligned to 4
 * elements, else two. */
int oth_step_vs_observe(oth_env *env, int32_t opponent_policy, const int32_t *actions, const int8_t *protagonist,
                        int32_t *rewards, uint8_t *dones, int32_t *plies, int32_t layout, int32_t dtype, void *obs,
                        oth_stream_t stream);

/* The search as a player: one colour's (or the embedded opponent's) move
 * chooser.  The struct is host memory, read during the call; its values are
 * baked into the launch, so the calls below stay capturable into a HIP graph.
 *
 * The searched move S(board, p).  With e the board's number of empty squares,
 * d = e if e <= p.endgame_empties, else d = p.depth.  oth_search's computation
 * runs on the board with depth d and p's weights, mobility_weight,
 * terminal_weight and max_nodes (per root move); the root list is the board's
 * stored possible_moves.  Status DONE: S is `best`.  Status ABORTED: S is
 * oth_greedy_actions' move (the most flips, the lowest square of equals) and
 * the ply counts as a *fallback*.  With d = e every line reaches a game end, so
 * from endgame_empties squares on the move is oth_solve's `best` (a positive
 * terminal_weight does not change the argmax). */
typedef struct oth_search_policy {
    const int8_t *weights;     /* DEVICE int8[N*N], as oth_search takes it */
    int32_t depth;             /* [1, OTH_SEARCH_MAX_DEPTH] */
    int32_t mobility_weight;   /* [-127, 127] */
    int32_t terminal_weight;   /* [1, 32767] */
    int32_t endgame_empties;   /* [0, OTH_SEARCH_MAX_DEPTH] */
    uint64_t max_nodes;        /* [1, 2^32 - 1], per root move */
} oth_search_policy;

/* oth_step_policy with the policy's move replaced by S: black's plies use
 * *black, white's *white (the two may be the same pointer; neither may be
 * NULL).  Everything else is oth_step_policy's contract: a random move while
 * random-opening plies remain, drawn for ply g = ply counter + p; an already
 * terminated board gives action -1, done 1, reward 0; OTH_AUTO_RESET resets a
 * board after its terminal ply; the tallies are oth_counts'; the ply counter
 * advances by n_plies; inside a graph region the slot's ply offset is added.
 * Outputs are [n_plies][E], each may be NULL, every element of a non-NULL
 * output is written; fallbacks[p][e] is 1 where ply p of board e was an aborted
 * search played by greedy, else 0.  A live board with an empty stored mask
 * plays what oth_step_policy(OTH_POLICY_GREEDY) plays there (action -1).
 *
 * oth_reset_vs_search / oth_step_vs_search are oth_reset_vs / oth_step_vs with
 * the opponent's policy move replaced by S(board, *opponent); the control flow,
 * the draws (ply j of call c uses counter c*256 + j), the negated reward,
 * plies, both tallies, the reset_vs-style OTH_AUTO_RESET and the one ply
 * counter consumed per call are theirs.  fallbacks[e] (may be NULL) is the
 * number of the opponent's plies of this call that were fallbacks, the replies
 * of an auto-reset included.  For the observation, call oth_observe after it.
 *
 * One launch each (a wave per 8 boards, the boards' root moves over its
 * lanes); no call synchronises the host.  OTH_EINVAL, checked before the
 * handle is read and with nothing launched: a NULL handle, a NULL policy, NULL
 * weights inside a policy, a field out of range, n_plies < 1, NULL actions in
 * oth_step_vs_search. */
int oth_play_search(oth_env *env, const oth_search_policy *black, const oth_search_policy *white,
                    int32_t n_plies, int32_t *actions, int32_t *rewards, uint8_t *dones, uint8_t *fallbacks,
                    oth_stream_t stream);
int oth_reset_vs_search(oth_env *env, const oth_search_policy *opponent, const int8_t *protagonist,
                        const uint8_t *mask, oth_stream_t stream);
int oth_step_vs_search(oth_env *env, const oth_search_policy *opponent, const int32_t *actions,
                       const int8_t *protagonist, int32_t *rewards, uint8_t *dones, int32_t *plies,
                       int32_t *fallbacks, oth_stream_t stream);

/* The network as a player: one colour's (or the embedded opponent's) move
 * chooser is an oth_net network.  The struct is host memory, read during the
 * call; its values are baked into the launch, so the calls below stay capturable
 * into a HIP graph.
 *
 * The network's move P(board, p).  M is the board's stored possible_moves on
 * the board's squares (the root list S reads); z and prior[] are oth_net_eval's
 * logits and priors of the row (the board's black words, white words, the turn
 * bit of its meta, its stored legal words) with p.params and p.blob; D is the
 * number of discs on the board, popcount(black | white).
 *   D >= p.sample_discs: the move is the square of M with the largest z[a], the
 *     lowest square among equals.  No prior takes part: logits that differ by
 *     less than one step of a prior still decide.
 *   D <  p.sample_discs: a draw in proportion to the priors, oth_puct_pick's
 *     rule on prior[].  P = the sum of prior[a] over M (at least 1: the largest
 *     logit's prior is at least 65535 / |M|); u = word 0 of the Philox4x32-10
 *     block with key `seed` and counter words (id, g lo, g hi, 7) -- purpose 7,
 *     a purpose of its own beside the seven of the draws above -- with id the
 *     global env id (env_id_base + e mod 2^32) and g the ply's global index, the
 *     one a random move of that ply would be drawn with: ply counter + p in
 *     oth_play_net, c*256 + j in the vs calls; r = floor(u P / 2^32); the move
 *     is the first square of M in ascending order whose cumulative prior exceeds
 *     r.  A legal square of prior 0 is never drawn.
 * sample_discs = 0 is a deterministic player, 257 always samples; on 8 x 8,
 * sample_discs = 12 samples the first eight discs placed. */
#define OTH_NET_SAMPLE_DISCS_MAX 257
typedef struct oth_net_policy {
    oth_net_params params;   /* as oth_net_eval takes them */
    const void *blob;        /* DEVICE: oth_net_pack's bytes, 16-byte aligned */
    uint64_t blob_bytes;     /* at least what oth_net_blob_bytes reports */
    int32_t sample_discs;    /* [0, 257] */
} oth_net_policy;

/* oth_play_net: oth_step_policy with the policy's move replaced by P: black's
 * plies use *black, white's *white (the two may be the same pointer; neither
 * may be NULL).  Everything else is oth_step_policy's contract, as
 * oth_play_search states it: a random move while random-opening plies remain,
 * drawn for ply g = ply counter + p; an already terminated board gives action
 * -1, done 1, reward 0; a live board with an empty stored mask plays action -1;
 * OTH_AUTO_RESET resets a board after its terminal ply; the tallies are
 * oth_counts'; the ply counter advances by n_plies; inside a graph region the
 * slot's ply offset is added.  Outputs are [n_plies][E], each may be NULL.
 * The two networks must have the same width (the kernel's accumulators are a
 * compile-time width / 64): another width is OTH_EINVAL.  layers, the shifts and
 * the weights may differ.
 *
 * oth_reset_vs_net / oth_step_vs_net are oth_reset_vs / oth_step_vs with the
 * opponent's policy move replaced by P(board, *opponent), in a reset's replies
 * too; the control flow, the draws (ply j of call c uses counter c*256 + j), the
 * negated reward, plies, both tallies, the reset_vs-style OTH_AUTO_RESET and the
 * one ply counter consumed per call are theirs, exactly as the _search calls
 * state it.  For the observation, call oth_observe after it.
 *
 * One launch each (a wave per 16 boards: a tile of rows on the matrix cores); no
 * call synchronises the host.  OTH_EINVAL, checked before the handle's device is
 * touched and with nothing launched: a NULL handle, a NULL policy, a NULL blob, a
 * field of params out of range for the handle's board size, blob_bytes below
 * what oth_net_blob_bytes reports, a blob that is not 16-byte aligned,
 * sample_discs outside [0, 257], two widths in oth_play_net, n_plies < 1, NULL
 * actions in oth_step_vs_net.  The host cannot read a blob: one packed for
 * another geometry or other shifts is found by the kernel, which then changes
 * nothing -- no board, no output, no tally (oth_net_eval's rule); the ply
 * counter has advanced all the same. */
int oth_play_net(oth_env *env, const oth_net_policy *black, const oth_net_policy *white, int32_t n_plies,
                 int32_t *actions, int32_t *rewards, uint8_t *dones, oth_stream_t stream);
int oth_reset_vs_net(oth_env *env, const oth_net_policy *opponent, const int8_t *protagonist, const uint8_t *mask,
                     oth_stream_t stream);
int oth_step_vs_net(oth_env *env, const oth_net_policy *opponent, const int32_t *actions, const int8_t *protagonist,
                    int32_t *rewards, uint8_t *dones, int32_t *plies, oth_stream_t stream);

/* The convolutional network as a player: one colour's (or the embedded
 * opponent's) move chooser is an oth_cnet network.  The struct is host memory,
 * read during the call, as oth_net_policy is.
 *
 * The network's move is P(board, p) above, word for word, with "z and prior[]
 * are oth_cnet_eval's logits and priors of the row" in place of oth_net_eval's:
 * the same M, the same D, the same argmax and tie rule, the same draw (purpose
 * 7, counter words (id, g lo, g hi, 7), r = floor(u P / 2^32), the first square
 * whose cumulative prior exceeds r). */
typedef struct oth_cnet_policy {
    oth_cnet_params params;  /* as oth_cnet_eval takes them */
    const void *blob;        /* DEVICE: oth_cnet_pack's bytes, 16-byte aligned */
    uint64_t blob_bytes;     /* at least what oth_cnet_blob_bytes reports */
    int32_t sample_discs;    /* [0, OTH_NET_SAMPLE_DISCS_MAX] */
} oth_cnet_policy;

/* oth_play_cnet / oth_reset_vs_cnet / oth_step_vs_cnet are oth_play_net /
 * oth_reset_vs_net / oth_step_vs_net with that P: everything the comment on
 * oth_play_net states beside the move -- random-opening plies, terminated
 * boards, the empty stored mask's action -1, OTH_AUTO_RESET, both tallies, the
 * ply counter, the graph region's offset, the vs calls' phase order and their
 * c*256 + j counters -- holds unchanged.  The two networks of oth_play_cnet may
 * differ in blocks, in every shift and in the weights; they must have the same
 * `channels` (the kernel's compile-time parameter): another count is OTH_EINVAL.
 *
 * One launch each (a workgroup of four waves per 4, 2 or 1 boards: the board's
 * activations stay in its LDS); no call synchronises the host.  OTH_EINVAL,
 * checked before the handle's device is touched and with nothing launched: the
 * list of oth_play_net, with oth_cnet_eval's field ranges, oth_cnet_blob_bytes
 * for blob_bytes and "two channel counts" for "two widths".  A blob packed for
 * another geometry or other shifts (any of its first 32 bytes: both tags and the
 * 16 block shifts) is found by the kernel, which then changes nothing -- no
 * board, no output, no tally; the ply counter has advanced all the same. */
int oth_play_cnet(oth_env *env, const oth_cnet_policy *black, const oth_cnet_policy *white, int32_t n_plies,
                  int32_t *actions, int32_t *rewards, uint8_t *dones, oth_stream_t stream);
int oth_reset_vs_cnet(oth_env *env, const oth_cnet_policy *opponent, const int8_t *protagonist, const uint8_t *mask,
                      oth_stream_t stream);
int oth_step_vs_cnet(oth_env *env, const oth_cnet_policy *opponent, const int32_t *actions, const int8_t *protagonist,
                     int32_t *rewards, uint8_t *dones, int32_t *plies, oth_stream_t stream);

/* The n-tuple network as a player: one colour's (or the embedded opponent's)
 * move chooser is oth_search_ntuple's computation over an oth_ntuple network.
 * The struct is host memory, read during the call, as oth_search_policy is.
 *
 * The move T(board, p) is oth_search_policy's S, word for word, with
 * oth_search_ntuple's computation in place of oth_search's: with e the board's
 * number of empty squares, d = e if e <= p.endgame_empties, else d = p.depth;
 * the search runs on the board with depth d, p's params, plan, weights,
 * terminal_weight and max_nodes (per root move); the root list is the board's
 * stored possible_moves.  Status DONE: T is `best`.  Status ABORTED: T is
 * oth_greedy_actions' move and the ply counts as a fallback.
 *
 * Exploration comes before the search.  x = the Philox4x32-10 block with key
 * `seed` and counter words (id, g lo, g hi, 8) -- purpose 8, a purpose of its own
 * -- with id the global env id (env_id_base + e mod 2^32) and g the ply's global
 * index, exactly as oth_play_net defines it: ply counter + p in oth_play_ntuple,
 * c*256 + j in the vs calls.  The ply explores iff (x word 0 >> 16) < p.explore:
 * the move is then the k-th square of the stored mask in ascending order (from
 * 0), k = floor(x word 1 * count / 2^32) with count the mask's squares, and the
 * ply is no fallback.  explore = 0 never draws, explore = OTH_NTUPLE_EXPLORE_ONE
 * always explores; epsilon = explore / 65536.  The draw depends on the seed, the
 * global id and the ply alone: a sharded run equals the unsharded one. */
#define OTH_NTUPLE_EXPLORE_ONE 65536
typedef struct oth_ntuple_policy {
    oth_ntuple_params params;   /* as oth_ntuple_eval takes them */
    const void *plan;           /* DEVICE: oth_ntuple_plan's bytes, 8-byte aligned */
    uint64_t plan_bytes;        /* at least what oth_ntuple_plan_bytes reports */
    const int32_t *weights;     /* DEVICE int32[n_weights + 1] */
    uint64_t weight_count;      /* at least what oth_ntuple_weight_count reports */
    int32_t depth;              /* [1, OTH_SEARCH_MAX_DEPTH] */
    int32_t terminal_weight;    /* [1, 32767] */
    int32_t endgame_empties;    /* [0, OTH_SEARCH_MAX_DEPTH] */
    int32_t explore;            /* [0, 65536]: epsilon in 1/65536 */
    uint64_t max_nodes;         /* [1, 2^32 - 1], per root move */
} oth_ntuple_policy;

/* The TD(0) rows of oth_play_ntuple's plies, from the same launch: host memory
 * holding DEVICE addresses, all four required.  For ply p of board e, learn is 1
 * iff the board was live before the ply, had a non-empty stored mask, the ply
 * was neither a random-opening ply nor an exploring one, and its search was
 * DONE.  For such a row boards / meta are the row before the ply in the exchange
 * format (the handle's meta word; only its turn bit matters to the oth_ntuple
 * calls), and targets is taken from that row's mover's side, under that mover's
 * colour's policy, from the position the ply leaves before any auto-reset:
 *   the game is over:              32768 * sign(mover's discs - opponent's discs);
 *   the same side moves again:     +H(next row)   (the opponent had to pass);
 *   otherwise:                     -H(next row),
 * with H oth_ntuple_eval's value of the next row.  Every other element of the
 * four arrays is written as 0.  The weights are read as they are when the launch
 * runs and are not changed by it. */
typedef struct oth_ntuple_td {
    uint64_t *boards;   /* [n_plies][E][2W] */
    uint16_t *meta;     /* [n_plies][E]     */
    int32_t *targets;   /* [n_plies][E]     */
    uint8_t *learn;     /* [n_plies][E]     */
} oth_ntuple_td;

/* oth_play_ntuple / oth_reset_vs_ntuple / oth_step_vs_ntuple are oth_play_search
 * / oth_reset_vs_search / oth_step_vs_search with S replaced by T: everything the
 * comment on oth_play_search states beside the move -- random-opening plies,
 * terminated boards (action -1, done 1, reward 0), the empty stored mask's
 * action -1, OTH_AUTO_RESET, both tallies, the ply counter, the graph region's
 * ply offset, the vs calls' phase order and their c*256 + j counters, fallbacks
 * per ply (play) and per board (step_vs), "every element of a non-NULL output is
 * written" -- holds unchanged.  The two sides of oth_play_ntuple may differ in
 * everything: tuples, value_shift, weights, depth.  td may be NULL (no rows).
 *
 * One launch each (a wave per 8 boards, the boards' root moves over its lanes,
 * both plans in its LDS); no call synchronises the host; each is capturable into
 * a HIP graph.  OTH_EINVAL, with nothing launched: a NULL handle, policy, plan
 * or weights; a field of params out of range for the handle's board size;
 * plan_bytes or weight_count below what oth_ntuple_plan_bytes /
 * oth_ntuple_weight_count report; a plan that is not 8-byte aligned; depth,
 * terminal_weight, endgame_empties, explore or max_nodes out of range; n_plies <
 * 1; NULL actions in oth_step_vs_ntuple; a td with a NULL member.  The host
 * cannot read a plan: one that is not the plan of the policy's params is found by
 * the kernel, which then changes nothing -- no board, no output, no tally
 * (oth_play_net's rule); the ply counter has advanced all the same. */
int oth_play_ntuple(oth_env *env, const oth_ntuple_policy *black, const oth_ntuple_policy *white, int32_t n_plies,
                    int32_t *actions, int32_t *rewards, uint8_t *dones, uint8_t *fallbacks, const oth_ntuple_td *td,
                    oth_stream_t stream);
int oth_reset_vs_ntuple(oth_env *env, const oth_ntuple_policy *opponent, const int8_t *protagonist,
                        const uint8_t *mask, oth_stream_t stream);
int oth_step_vs_ntuple(oth_env *env, const oth_ntuple_policy *opponent, const int32_t *actions,
                       const int8_t *protagonist, int32_t *rewards, uint8_t *dones, int32_t *plies,
                       int32_t *fallbacks, oth_stream_t stream);

/* oth_ntuple_update with a row mask: mask uint8[R] is a device input, NULL means
 * every row.  Where mask[r] == 0, d_r = 0: deltas[r] = 0 is written and nothing
 * is added for the row.  Everything else is oth_ntuple_update's contract.  A
 * TD(0) step over n plies is then two calls with no host synchronisation:
 * oth_play_ntuple with td, then this call on the n_plies * E rows with td.learn
 * as the mask.  The weights are frozen during the play launch, so the result
 * stays an exact, order-independent function of the inputs. */
int oth_ntuple_update_masked(int32_t board_size, int32_t n_rows, const oth_ntuple_params *params, const void *plan,
                             uint64_t plan_bytes, int32_t *weights, uint64_t weight_count, const uint64_t *boards,
                             const uint16_t *meta, const int32_t *targets, const uint8_t *mask, int32_t rate,
                             int32_t rate_shift, int32_t *deltas, oth_stream_t stream);

/* possible_moves of every env as masks uint64[E][W] (othello.py:242, :270, :466). */
int oth_legal(oth_env *env, uint64_t *out, oth_stream_t stream);

/* get_possible_actions(board) (othello.py:313-343), stateless: n canonical
 * boards given as mover / opponent masks uint64[n][W] -> uint64[n][W]. */
int oth_legal_moves(int32_t board_size, int32_t n, const uint64_t *mover, const uint64_t *opp, uint64_t *out,
                    oth_stream_t stream);

/* GreedyPolicy.get_action (simple_policies.py:69-92) for the side to move in
 * every env: argmax over possible_moves of the discs flipped, lowest square
 * on ties; -1 where possible_moves is empty.  Out int32[E]. */
int oth_greedy_actions(oth_env *env, int32_t *out, oth_stream_t stream);

/* The move of a deterministic scripted policy (OTH_POLICY_GREEDY or
 * OTH_POLICY_MAXIMIN(d): MaxiMinPolicy(d).get_action, simple_policies.py:157-163)
 * for the side to move in every env; -1 where possible_moves is empty.
 * MaxiMin(d >= 3) searches each board with a whole wave (the root's moves and
 * their replies spread over the lanes); above OTH_MAXIMIN_LEAF_BUDGET estimated
 * leaves (position-aware, see there) the call is refused (OTH_EINVAL) before
 * anything is launched. */
int oth_policy_actions(oth_env *env, int32_t policy, int32_t *out, oth_stream_t stream);

/* Observations: layout OTH_OBS_*, dtype OTH_I8..OTH_BF16, out (E, planes, N, N). */
int oth_observe(oth_env *env, int32_t layout, int32_t dtype, void *out, oth_stream_t stream);

/* Copy the state out / in (exchange format above).  In oth_set_state any of
 * the three sources may be NULL (left unchanged): set_board_state
 * (othello.py:380-389) replaces only the boards. */
int oth_get_state(oth_env *env, uint64_t *boards, uint16_t *meta, uint64_t *legal, oth_stream_t stream);
int oth_set_state(oth_env *env, const uint64_t *boards, const uint16_t *meta, const uint64_t *legal,
                  oth_stream_t stream);

/* set_player_turn (othello.py:464-466): turn (+1 white / -1 black) for every
 * env (or where mask[e] != 0), then recompute possible_moves. */
int oth_set_player_turn(oth_env *env, int32_t turn, const uint8_t *mask, oth_stream_t stream);

/* count_disks (othello.py:468-471): out int32[E][2] = (white_cnt, black_cnt). */
int oth_count_disks(oth_env *env, int32_t *out, oth_stream_t stream);

/* Win/draw/loss tally of games finished by oth_step / oth_step_policy since
 * the last reset of the counters: out int64[3] = {black wins, draws, white
 * wins} (device pointer).  reset != 0 zeroes the counters after the copy. */
int oth_counts(oth_env *env, int64_t *out, int32_t reset, oth_stream_t stream);

/* The harnesses' tally (run.py:100-130, the README's wins / draws / loses) of
 * games finished by oth_step_vs, from each board's protagonist's side: out
 * int64[3] = {protagonist wins, draws, protagonist losses} (device pointer);
 * reset != 0 zeroes the counters after the copy. */
int oth_counts_vs(oth_env *env, int64_t *out, int32_t reset, oth_stream_t stream);

/* Masked categorical over each board's legal squares (policy head of the
 * learners; replaces the per-sample loops of
 * pytorch_a2c_ppo_acktr_gail/a2c_ppo_acktr/model.py:60-99 Policy.act,
 * model.py:156-178 Policy.evaluate_actions and ppo.py:228-298 PPO.get_action).
 * n boards: logits float32 rows of N*N with row stride ld (elements), legal
 * uint64[n][W] (e.g. oth_legal's output), device pointers.
 *   OTH_MASKED_SAMPLE: action = the first legal square whose cumulative
 *     softmax mass exceeds u * total, u = uniforms[e] in [0,1) if uniforms is
 *     non-NULL, else a Philox draw keyed (seed, id_base + e, counter);
 *   OTH_MASKED_MODE: action = the lowest legal square of the largest logit;
 *   OTH_MASKED_EVAL: actions is an INPUT.
 * log_probs[e] = log softmax over the legal squares at the action (0 when the
 * board has no legal move or the action is not one of them, model.py:69-71,
 * :165); entropy[e] = entropy of the masked distribution (0 with no legal
 * move).  A board without legal moves samples action 0 (model.py:69-71).
 * log_probs / entropy may be NULL.  Logits must be finite. */
int oth_masked_sample(int32_t board_size, int32_t n, const float *logits, int64_t ld, const uint64_t *legal,
                      const float *uniforms, uint64_t seed, uint32_t id_base, uint64_t counter, int32_t mode,
                      int32_t *actions, float *log_probs, float *entropy, oth_stream_t stream);

/* oth_masked_sample over the handle's own boards and possible_moves, keyed
 * by the handle's seed and env ids. */
int oth_sample_actions(oth_env *env, const float *logits, int64_t ld, const float *uniforms, uint64_t counter,
                       int32_t mode, int32_t *actions, float *log_probs, float *entropy, oth_stream_t stream);

/* One ply of the learners' loop in one launch: oth_sample_actions (mode
 * OTH_MASKED_SAMPLE or OTH_MASKED_MODE, optionally | OTH_MASKED_FULL_ENTROPY)
 * over the handle's possible_moves, then oth_step with the chosen actions
 * (Policy.act model.py:60-99 / PPO.get_action ppo.py:228-262, then
 * OthelloBaseEnv.step othello.py:412-462).  Results are bit-identical to the
 * two calls.  Out: actions int32[E] (required), log_probs / entropy float[E],
 * rewards int32[E], dones uint8[E] (each may be NULL).  Advances the ply
 * counter by one; `counter` is the sample counter as in oth_sample_actions. */
int oth_sample_step(oth_env *env, const float *logits, int64_t ld, const float *uniforms, uint64_t counter,
                    int32_t mode, int32_t *actions, float *log_probs, float *entropy, int32_t *rewards,
                    uint8_t *dones, oth_stream_t stream);

/* oth_sample_step, then the observation of the stepped boards (layout, dtype
 * as oth_observe: e.g. OTH_OBS_MAKE_STATE in OTH_F32, the learners' next input,
 * util.py:48-74) into obs in the same call: bit-identical to oth_sample_step +
 * oth_observe.  One launch for N*N % 4 == 0 with obs aligned to 4 elements. */
int oth_sample_step_observe(oth_env *env, const float *logits, int64_t ld, const float *uniforms, uint64_t counter,
                            int32_t mode, int32_t *actions, float *log_probs, float *entropy, int32_t *rewards,
                            uint8_t *dones, int32_t layout, int32_t dtype, void *obs, oth_stream_t stream);

/* One board's state in the reference's terms, as the single-board drop-in
 * classes (OthelloBaseEnv / SimpleOthelloEnv / OthelloEnv, othello.py:21-501;
 * BASELINE config 1) return it after every call.  W used words per colour. */
#define OTH_RECORD_MAX_WORDS 4
#define OTH_RECORD_GREEDY 2       /* oth_step_sync's `step` bit: also compute the record's greedy move */
#define OTH_RECORD_NO_GREEDY (-2) /* the record's greedy field when that bit was not given */
#define OTH_RECORD_MAX_SQUARES 256
typedef struct oth_record {
    uint64_t black[OTH_RECORD_MAX_WORDS]; /* the board (exchange format) */
    uint64_t white[OTH_RECORD_MAX_WORDS];
    uint64_t legal[OTH_RECORD_MAX_WORDS]; /* possible_moves (stale on terminal plies, as the reference's) */
    uint32_t seq;                         /* the call's sequence number (written last) */
    uint16_t meta;                        /* exchange-format meta: player_turn, terminated, winner */
    uint8_t done;                         /* the step's done (0 without a step) */
    uint8_t planes;                       /* observation planes in obs: 1, or 2 with the legal plane */
    int32_t reward;                       /* the step's reward (0 without a step) */
    int32_t white_cnt, black_cnt;         /* count_disks (othello.py:468-471) */
    int32_t greedy;                       /* GreedyPolicy.get_action for the side to move (simple_policies.py:69-92);
                                             -1 without a possible move; OTH_RECORD_NO_GREEDY unless the call
                                             asked for it (OTH_RECORD_GREEDY) */
    int8_t obs[2 * OTH_RECORD_MAX_SQUARES];   /* get_observation() (othello.py:363-378): planes x N x N */
    int8_t board_state[OTH_RECORD_MAX_SQUARES]; /* board_state (othello.py:257): white +1, black -1 */
} oth_record;

/* The single-board drop-in path in one launch and one wait: if step & 1,
 * OthelloBaseEnv.step (othello.py:412-462) of board `board` with the host value
 * `action` (any int: not in possible_moves takes the invalid path; a
 * terminated board is left as it is and reports done, as oth_step), then the
 * board's record (layout OTH_OBS_BOARD or OTH_OBS_BOARD_LEGAL for obs) is
 * written by the same kernel into a mapped host buffer the handle owns, and the
 * call returns once it has landed: *out points at it until the next call on
 * this handle.  step & 1 == 0 only records (after reset / set_state /
 * set_player_turn).  step & OTH_RECORD_GREEDY also computes GreedyPolicy's move
 * for the side to move (one lane's bit-plane flip counts: about 0.5 us of the
 * call, so only when a greedy policy reads the record). */
int oth_step_sync(oth_env *env, int32_t board, int32_t step, int32_t action, int32_t layout,
                  const oth_record **out, oth_stream_t stream);

/* Global ply counter of the handle: the Philox counter of the next eager ply
 * (random policy, openings, device opponents).  Host value only; setting it
 * does not touch graph regions' counter ranges (below). */
uint64_t oth_ply_counter(const oth_env *env);
int oth_set_ply_counter(oth_env *env, uint64_t ply);

/* HIP-graph regions (no reference counterpart: the reference has no device).
 * Every entry point only enqueues kernels on `stream`, so a region of calls can
 * be captured and replayed.  The Philox counters a capture bakes in are host
 * values; to make every replay draw fresh numbers without reusing any counter
 * of eager calls or of other graphs, each region owns a disjoint counter range:
 *   oth_graph_begin: opens region k (k = 1 .. OTH_GRAPH_SLOTS-1, *slot = k);
 *     until oth_graph_end the handle's ply counter runs from
 *     k << OTH_GRAPH_COUNTER_SHIFT and launches add the device offsets of slot k;
 *   oth_graph_end: closes it, restores the eager ply counter, *d_ply = plies
 *     the region consumed; if enqueue != 0 it enqueues (as the region's last
 *     node) the advance of slot k's offsets by (d_ply, d_sample), so replay r
 *     draws the counters (k << SHIFT) + r * d + j.  d_sample is what the caller's
 *     sample counter (oth_sample_actions) consumed inside the region, whose
 *     range must start at k << SHIFT as well.
 *   oth_graph_offsets: slot k's (ply, sample) offsets; synchronises the device
 *     (never call it while a capture is active).
 *   oth_graph_release: gives slot k back (its graph is dropped, or its capture
 *     failed); oth_graph_begin hands out the lowest free slot.  The slot's
 *     offsets are kept, so a later region on it still draws fresh counters.
 * Eager launches use slot 0, always 0. */
#define OTH_GRAPH_SLOTS 64
#define OTH_GRAPH_COUNTER_SHIFT 40
int oth_graph_begin(oth_env *env, int32_t *slot);
int oth_graph_end(oth_env *env, uint64_t d_sample, int32_t enqueue, uint64_t *d_ply, oth_stream_t stream);
int oth_graph_offsets(const oth_env *env, int32_t slot, uint64_t out[2]);
int oth_graph_release(oth_env *env, int32_t slot);

/* Handle geometry: n_envs, board_size, W. */
int oth_shape(const oth_env *env, int32_t *n_envs, int32_t *board_size, int32_t *words);

/* Message of the last failing call on this thread ("" if none). */
const char *oth_last_error(void);

/* Library version string. */
const char *oth_version(void);

#ifdef __cplusplus
}
#endif
#endif /* OTHELLO_MI355X_H */
