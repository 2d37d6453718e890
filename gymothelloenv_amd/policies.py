"""Scripted policies with the reference's protocol (simple_policies.py).

`reset(env)` (unwrapping `env.env` like simple_policies.py:28-32),
`get_action(obs)`, `get_test_action(obs)`, optional `seed(seed)`.

RandomPolicy draws exactly like simple_policies.py:37-41 (np.random.RandomState
index into possible_moves), so seeded games match the reference move for move.
GreedyPolicy and MaxiMinPolicy ask the device kernels (oth_policy_actions) for
the move of simple_policies.py:69-92 / :98-163 -- greedy: the move flipping the
most discs, lowest square on ties; maximin: the depth-limited max-min search
with the reference's pass handling -- instead of simulating every candidate on
copied envs.
"""
import numpy as np

from . import _lib as L
from .othello import WHITE_DISK
from .vec_env import SearchConfig  # noqa: F401  (SearchPolicy's batched counterpart: the search played on the device)
from .ntuple import NTuplePlayer  # noqa: F401  (NTuplePolicy's batched counterpart: the n-tuple net played on the device)

PROTAGONIST_TURN = 1  # simple_policies.py:8-9
OPPONENT_TURN = -1


def _base(env):
    return env.env if hasattr(env, 'env') else env


class RandomPolicy(object):
    """simple_policies.py:21-44"""

    def __init__(self, seed=0):
        self.rnd = np.random.RandomState(seed=seed)
        self.env = None

    def reset(self, env):
        self.env = _base(env)

    def seed(self, seed):
        self.rnd = np.random.RandomState(seed=seed)

    def get_action(self, obs):
        possible_moves = self.env.possible_moves
        ix = self.rnd.randint(0, len(possible_moves))
        return possible_moves[ix]

    def get_test_action(self, obs):
        return self.get_action(obs)


class GreedyPolicy(object):
    """simple_policies.py:57-95: the move the device computed for the side to move
    (the bit-plane flip counts of every square, lowest square on ties) -- read
    from the board's record, which the launch of the last step / reset wrote
    (oth_step_sync): no device call of its own."""

    def __init__(self):
        self.env = None

    def reset(self, env):
        self.env = _base(env)
        self.env._greedy_bit = L.OTH_RECORD_GREEDY  # the env's records carry the greedy move from now on

    def get_action(self, obs):
        obs = np.asarray(obs)
        if obs.ndim == 3 and obs.shape[0] == 4:  # make_state obs: same turn check as undo_state
            assert int((self.env.player_turn + 1) / 2) == int(obs[2][0][0])
        a = self.env._greedy_move()
        if a < 0:
            raise ValueError('no possible moves')
        return a

    def get_test_action(self, obs):
        return self.get_action(obs)


class MaxiMinPolicy(object):
    """simple_policies.py:98-163, searched on the device.

    max_search_depth <= 0: the reference's search stops at the root (depth 0 >=
    max_search_depth, :117-126) and get_action returns None -- no device call.
    1 .. OTH_MAXIMIN_MAX_DEPTH (10): the device search -- depth 3 and deeper with
    a whole wave per board (the root's moves and their replies spread over the
    lanes, maximin_wave.hpp).  Deeper: the same search at depth = the board's
    empty squares, which it equals (every level places a disc), once the board
    has at most 10 empty squares; earlier in the game such a move raises
    (VecOthelloEnv.policy_actions).  The search is exponential in the depth: about b**depth
    leaves for b moves per position (8x8 middle games: b ~ 10), fewer late in the
    game (at most e! for e empty squares).  The C ABI refuses calls estimated
    above OTH_MAXIMIN_LEAF_BUDGET leaves (1.7e10), bounded by the board's own
    empty squares, so one 8x8 board searches depth 10 from 10 empty squares on;
    DEEP_WARN_LEAVES bounds what runs without a warning."""

    DEEP_WARN_LEAVES = 10 ** 6

    def __init__(self, max_search_depth=1):
        self.env = None
        self.max_search_depth = int(max_search_depth)

    def reset(self, env):
        self.env = _base(env)
        n = getattr(self.env, "board_size", 8)
        b = max(2, n * n // 6)  # a typical middle-game move count (8x8: ~10)
        if self.max_search_depth > 0 and b ** self.max_search_depth > self.DEEP_WARN_LEAVES:
            import warnings
            warnings.warn("MaxiMinPolicy(%d) on %dx%d boards searches up to ~%.0e leaves per middle-game move "
                          "(one wave of the GPU per board): such moves can take seconds, or be refused above the "
                          "C ABI's leaf budget; late-game moves (few empty squares) search far fewer" %
                          (self.max_search_depth, n, n, float(b ** self.max_search_depth)), RuntimeWarning)

    def get_action(self, obs):
        if self.max_search_depth <= 0:
            return None  # search(depth=0) returns (count, None) at once (:117-126)
        vec = self.env._vec
        self.env._sync()
        a = int(vec.policy_actions("maximin%d" % self.max_search_depth).cpu()[0])
        return a if a >= 0 else None  # the reference's search returns no move then (:117-126, :157-163)

    def get_test_action(self, obs):
        return self.get_action(obs)


class MonteCarloPolicy(object):
    """Flat Monte-Carlo move selection (no reference counterpart: the rung after
    MaxiMinPolicy): the possible move whose n_playouts random games, played on
    the device (oth_playouts, per move), end best for the side to move -- the
    largest wins - losses, lowest square on ties.  Playouts are keyed by `seed`
    and a call counter that moves on with every move, so a seeded policy
    replays its games move for move."""

    def __init__(self, n_playouts=64, seed=0):
        self.env = None
        self.n_playouts = int(n_playouts)
        self._seed = int(seed)
        self.counter = 0

    def reset(self, env):
        self.env = _base(env)

    def seed(self, seed):
        self._seed = int(seed)
        self.counter = 0

    def get_action(self, obs):
        vec = self.env._vec
        self.env._sync()
        a = int(vec.playout_actions(self.n_playouts, seed=self._seed, counter=self.counter).cpu()[0])
        self.counter += 1
        if a < 0:
            raise ValueError('no possible moves')
        return a

    def get_test_action(self, obs):
        return self.get_action(obs)


class MCTSPolicy(object):
    """Monte-Carlo tree search move selection (no reference counterpart: the rung
    after MonteCarloPolicy): the most visited root move of a UCT-style tree search
    on the device (oth_mcts) with `iterations` descents, `playouts` random games
    per evaluated node and exploration constant c.  Playouts are keyed by `seed`
    and a call counter that moves on with every move, so a seeded policy replays
    its games move for move."""

    def __init__(self, iterations=256, playouts=8, c=1.0, seed=0):
        self.env = None
        self.iterations, self.playouts, self.c = int(iterations), int(playouts), float(c)
        self._seed = int(seed)
        self.counter = 0

    def reset(self, env):
        self.env = _base(env)

    def seed(self, seed):
        self._seed = int(seed)
        self.counter = 0

    def get_action(self, obs):
        vec = self.env._vec
        self.env._sync()
        a = int(vec.mcts_actions(self.iterations, playouts=self.playouts, c=self.c, seed=self._seed,
                                 counter=self.counter).cpu()[0])
        self.counter += 1
        if a < 0:
            raise ValueError('no possible moves')
        return a

    def get_test_action(self, obs):
        return self.get_action(obs)


class PUCTPolicy(object):
    """Network-guided tree search move selection (no reference counterpart: the
    rung after MCTSPolicy): the most visited root move of `simulations` simulations
    of VecOthelloEnv.puct_search, whose leaves `evaluate(leaves) -> (logits, values)`
    judges -- a policy and value network, or one of the evaluators that need none
    (None: playout_evaluator(8, seed), which replays its games move for move).  c is
    the exploration constant; simulations >= 2 (the first evaluates the root alone).
    leaves_per_board=K > 1 searches with K leaves per launch under virtual loss
    (puct_search's keyword): about simulations / K calls of evaluate, on K rows."""

    def __init__(self, evaluate=None, simulations=128, c=1.25, seed=0, leaves_per_board=1):
        self.env = None
        self.simulations, self.c = int(simulations), float(c)
        self.leaves_per_board = int(leaves_per_board)
        if not 1 <= self.leaves_per_board <= 64:
            raise ValueError("leaves_per_board must be in [1, 64]")
        self._seed = int(seed)
        self._own = evaluate is None
        self.evaluate = evaluate
        self.counter = 0
        if self.simulations < 2:
            raise ValueError("simulations must be >= 2: the first evaluates the root alone")

    def reset(self, env):
        self.env = _base(env)

    def seed(self, seed):
        self._seed = int(seed)
        self.counter = 0
        if self._own:
            self.evaluate = None

    def get_action(self, obs):
        vec = self.env._vec
        self.env._sync()
        if self.evaluate is None:
            from .vec_env import playout_evaluator
            self.evaluate = playout_evaluator(8, seed=self._seed)
        kw = dict(leaves_per_board=self.leaves_per_board) if self.leaves_per_board != 1 else {}
        a = int(vec.puct_actions(self.evaluate, self.simulations, c=self.c, **kw).cpu()[0])
        self.counter += 1
        if a < 0:
            raise ValueError('no possible moves')
        return a

    def get_test_action(self, obs):
        return self.get_action(obs)


class SolverPolicy(object):
    """Perfect endgame play (no reference counterpart): once the board has at most
    max_empties empty squares the move is the exact solver's `best` (oth_solve: the
    move of the largest final disc difference under best play by both sides, lowest
    square on ties).  Wherever the solver gives no exact answer -- more empty
    squares (SKIPPED), or a search over its node budget (ABORTED) -- `fallback`
    moves instead: GreedyPolicy() by default, or any policy of this protocol."""

    def __init__(self, max_empties=10, fallback=None):
        self.env = None
        self.max_empties = int(max_empties)
        self.fallback = fallback if fallback is not None else GreedyPolicy()

    def reset(self, env):
        self.env = _base(env)
        self.fallback.reset(env)

    def seed(self, seed):
        if hasattr(self.fallback, 'seed'):
            self.fallback.seed(seed)

    def get_action(self, obs):
        vec = self.env._vec
        self.env._sync()
        best, status = vec.solve(max_empties=self.max_empties, best=True, status=True)[1:]
        if int(status.cpu()[0]) == L.OTH_SOLVE_EXACT:
            return int(best.cpu()[0])
        return self.fallback.get_action(obs)

    def get_test_action(self, obs):
        return self.get_action(obs)


class SearchPolicy(object):
    """Depth-limited alpha-beta over weighted squares and mobility (no reference
    counterpart: the fixed middle-game opponent): the move is oth_search's `best`
    at `depth` with `weights` (None: default_search_weights), `mobility` and
    `terminal` as VecOthelloEnv.search takes them.  With solve_empties > 0 a board
    with at most that many empty squares goes to the exact solver first (oth_solve)
    and the search moves where the solver does not answer EXACT.  Where the search
    runs over its node budget (ABORTED) GreedyPolicy moves, as for SolverPolicy."""

    def __init__(self, depth=4, weights=None, mobility=0, terminal=64, solve_empties=0):
        self.env = None
        self.depth, self.weights, self.mobility, self.terminal = int(depth), weights, int(mobility), int(terminal)
        self.solve_empties = int(solve_empties)
        self.fallback = GreedyPolicy()

    def reset(self, env):
        self.env = _base(env)
        self.fallback.reset(env)

    def get_action(self, obs):
        vec = self.env._vec
        self.env._sync()
        if self.solve_empties > 0:
            best, status = vec.solve(max_empties=self.solve_empties, best=True, status=True)[1:]
            if int(status.cpu()[0]) == L.OTH_SOLVE_EXACT:
                return int(best.cpu()[0])
        best, status = vec.search(self.depth, self.weights, mobility=self.mobility, terminal=self.terminal,
                                  best=True, status=True)[1:]
        if int(status.cpu()[0]) == L.OTH_SEARCH_DONE:
            return int(best.cpu()[0])
        return self.fallback.get_action(obs)

    def get_test_action(self, obs):
        return self.get_action(obs)


class NTuplePolicy(object):
    """Depth-limited alpha-beta over an n-tuple network (no reference counterpart: the
    learned counterpart of SearchPolicy): the move is oth_search_ntuple's `best` at
    `depth` over `net` (an ntuple.NTupleNet), a game end valued by `terminal`.  Where
    the search runs over its node budget (ABORTED) GreedyPolicy moves, as for
    SearchPolicy.

    `net` may be an ntuple.NTuplePlayer instead: the move is then
    VecOthelloEnv.play_ntuple's for the board, computed by the same kernel -- the
    player's depth, endgame_empties, budget and exploring draws -- on a one-board
    scratch env that plays one ply of it, as NetPolicy does; seed(seed) keys the
    scratch env's draws."""

    def __init__(self, net, depth=1, terminal=64, seed=0):
        self.env = None
        self.player = net if getattr(net, "kind", None) == "ntuple" else None
        self.net = net.net if self.player is not None else net
        self.depth, self.terminal = int(depth), int(terminal)
        self.fallback = GreedyPolicy()
        self._seed = int(seed)
        self._scratch = None

    def reset(self, env):
        self.env = _base(env)
        self.fallback.reset(env)

    def seed(self, seed):
        if seed is not None and int(seed) != self._seed:
            self._seed = int(seed)
            self._scratch = None

    def _player_action(self):
        from .vec_env import VecOthelloEnv
        vec = self.env._vec
        if self._scratch is None or self._scratch.board_size != vec.board_size:
            self._scratch = VecOthelloEnv(1, board_size=vec.board_size, sudden_death_on_invalid_move=False,
                                          seed=self._seed, device=vec.device)
        self._scratch.set_state(*vec.get_state())
        a = int(self._scratch.play_ntuple(self.player, n_plies=1)[0].cpu()[0, 0])
        if a < 0:
            raise ValueError('no possible moves')
        return a

    def get_action(self, obs):
        vec = self.env._vec
        self.env._sync()
        if self.player is not None:
            return self._player_action()
        best, status = vec.search_ntuple(self.depth, self.net, terminal=self.terminal, best=True, status=True)[1:]
        if int(status.cpu()[0]) == L.OTH_SEARCH_DONE:
            return int(best.cpu()[0])
        return self.fallback.get_action(obs)

    def get_test_action(self, obs):
        return self.get_action(obs)


class NetPolicy(object):
    """A network as a player (no reference counterpart; the frozen-network opponent
    of self-play learners): the move is VecOthelloEnv.play_net's for the board --
    the legal square of the largest logit of `net` (a DeviceNet or a DeviceConvNet), the lowest square
    of equals, and a draw from the priors while the board holds fewer than
    `sample_discs` discs.  The move is computed by the same kernel: the board is
    copied to a one-board scratch env, which plays one ply of NetPlayer(net,
    sample_discs); seed(seed) keys the scratch env's draws."""

    def __init__(self, net, sample_discs=0, seed=0):
        from .net import NetPlayer
        self.env = None
        self.player = NetPlayer(net, sample_discs)
        self._seed = int(seed)
        self._scratch = None

    def reset(self, env):
        self.env = _base(env)

    def seed(self, seed):
        if seed is not None and int(seed) != self._seed:
            self._seed = int(seed)
            self._scratch = None

    def get_action(self, obs):
        from .vec_env import VecOthelloEnv
        vec = self.env._vec
        self.env._sync()
        if self._scratch is None or self._scratch.board_size != vec.board_size:
            self._scratch = VecOthelloEnv(1, board_size=vec.board_size, sudden_death_on_invalid_move=False,
                                          seed=self._seed, device=vec.device)
        self._scratch.set_state(*vec.get_state())
        a = int(self._scratch.play_net(self.player, n_plies=1)[0].cpu()[0, 0])
        if a < 0:
            raise ValueError('no possible moves')
        return a

    def get_test_action(self, obs):
        return self.get_action(obs)


__all__ = ['RandomPolicy', 'GreedyPolicy', 'MaxiMinPolicy', 'MonteCarloPolicy', 'MCTSPolicy', 'PUCTPolicy', 'SolverPolicy', 'SearchPolicy', 'NTuplePolicy', 'NetPolicy', 'PROTAGONIST_TURN', 'OPPONENT_TURN', 'WHITE_DISK']
