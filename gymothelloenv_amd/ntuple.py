"""The n-tuple network on the device (oth_ntuple_weight_count / oth_ntuple_plan /
oth_ntuple_eval / oth_ntuple_update / oth_search_ntuple; include/othello_mi355x.h
defines it in integers): a sum of look-up tables indexed by the contents of small
sets of squares, applied under the eight board symmetries.

    NTupleNet          the tables as an int32 device tensor the caller owns, with
                       evaluate (rows in the exchange format -> values), update (one
                       delta-rule step, exact and order-independent) and rate_for
    snake_tuples       random connected walks, the usual choice of tuples
    ntuple_evaluator   the net as an evaluator of VecOthelloEnv.puct_search
    NTuplePlayer       the net as a player (oth_play_ntuple, oth_reset_vs_ntuple,
                       oth_step_vs_ntuple): VecOthelloEnv.play_ntuple, an opponent of
                       reset_vs / step_vs, and with NTupleNet.td_play a TD(0) round in
                       two calls (TDRows: the rows the play launch recorded)

VecOthelloEnv.search_ntuple / search_ntuple_actions look ahead over the net, and
policies.NTuplePolicy plays it in the drop-in OthelloEnv."""
import collections
import ctypes

import numpy as np
import torch

from . import _lib as L


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def snake_tuples(board_size, count, length, seed=0):
    """`count` random connected walks of `length` distinct squares each: a walk starts
    on a random square and goes on to a random one of the eight neighbours not yet
    in it (a walk that gets stuck starts again).  Generated on the host with numpy's
    RandomState(seed): the same arguments give the same tuples.  A list of lists of
    squares r N + c."""
    n, count, length = int(board_size), int(count), int(length)
    if not 1 <= length <= min(L.OTH_NTUPLE_MAX_LENGTH, n * n) or not 1 <= count <= L.OTH_NTUPLE_MAX_TUPLES:
        raise ValueError("count must be in [1, 32] and length in [1, 8]")
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        walk = [int(rng.randint(n * n))]
        while len(walk) < length:
            r, c = divmod(walk[-1], n)
            nxt = [(r + dr) * n + c + dc for dr in (-1, 0, 1) for dc in (-1, 0, 1)
                   if (dr or dc) and 0 <= r + dr < n and 0 <= c + dc < n and (r + dr) * n + c + dc not in walk]
            if not nxt:
                break
            walk.append(nxt[int(rng.randint(len(nxt)))])
        if len(walk) == length:
            out.append(walk)
    return out


class NTupleNet(object):
    """An n-tuple network for N x N boards.  tuples: T lists of 1 .. 8 distinct squares
    (T <= 32); value_shift in [0, 24]: value = clamp(sum >> value_shift, -32768,
    32768), from the side to move, in units of 1 / 32768.

    `weights` is an int32 device tensor of `weight_count` = sum 3^len + 1 elements --
    tuple t's table at `offsets[t]`, the bias last -- zero at first; read it, write it
    in place, save it: it is a plain array and the learner's.  The plan (the eight
    transformed square lists a tuple) is made once on the host and kept on the
    device.  Every call is enqueued on the current stream and is capturable."""

    def __init__(self, board_size, tuples, value_shift=0, device=None):
        self._lib = L.load()
        self.board_size = n = int(board_size)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.tuples = [[int(a) for a in t] for t in tuples]
        self.value_shift = int(value_shift)
        if not 1 <= len(self.tuples) <= L.OTH_NTUPLE_MAX_TUPLES:
            raise ValueError("there must be 1 .. %d tuples" % L.OTH_NTUPLE_MAX_TUPLES)
        if any(not 1 <= len(t) <= L.OTH_NTUPLE_MAX_LENGTH for t in self.tuples):
            raise ValueError("a tuple has 1 .. %d squares" % L.OTH_NTUPLE_MAX_LENGTH)
        self.params = p = L.OthNtupleParams()
        p.tuples, p.value_shift = len(self.tuples), self.value_shift
        for t, sq in enumerate(self.tuples):
            p.length[t] = len(sq)
            for i, a in enumerate(sq):
                p.squares[t][i] = a
        count, need = ctypes.c_uint64(0), ctypes.c_uint64(0)
        L.check(self._lib.oth_ntuple_weight_count(n, ctypes.byref(p), ctypes.byref(count)), "oth_ntuple_weight_count")
        L.check(self._lib.oth_ntuple_plan_bytes(n, ctypes.byref(p), ctypes.byref(need)), "oth_ntuple_plan_bytes")
        host = torch.zeros(need.value // 8, dtype=torch.int64)
        L.check(self._lib.oth_ntuple_plan(n, ctypes.byref(p), _ptr(host), need.value), "oth_ntuple_plan")
        self.plan = host.to(self.device)
        self.plan_bytes = int(need.value)
        self.weight_count = int(count.value)
        self.offsets = [0]
        for t in self.tuples[:-1]:
            self.offsets.append(self.offsets[-1] + 3 ** len(t))
        self.weights = torch.zeros(self.weight_count, dtype=torch.int32, device=self.device)
        self._td_players = {}  # (depth, explore) -> td_play's NTuplePlayer

    def _rows(self, boards, meta):
        W = (self.board_size * self.board_size + 63) // 64
        R = int(meta.numel())
        bd = boards.to(device=self.device, dtype=torch.int64).contiguous()
        mt = meta.to(device=self.device, dtype=torch.int16).contiguous()
        if bd.numel() != R * 2 * W:
            raise ValueError("boards must have %d elements" % (R * 2 * W))
        return R, bd, mt

    def _weights(self):
        w = self.weights
        if w.dtype != torch.int32 or w.device != self.device or not w.is_contiguous() or w.numel() != self.weight_count:
            raise ValueError("weights must stay a contiguous int32 tensor of %d elements on %s" % (
                self.weight_count, self.device))
        return w

    def evaluate(self, boards, meta, sums=False):
        """Rows in the exchange format -- boards int64 (R, 2W), meta int16 (R,) -- to
        values int32 (R,), from each row's side to move; with sums=True (values, sums
        int64 (R,)), the sums before the shift and the clamp."""
        R, bd, mt = self._rows(boards, meta)
        w = self._weights()
        values = torch.empty(R, dtype=torch.int32, device=self.device)
        sm = torch.empty(R, dtype=torch.int64, device=self.device) if sums else None
        if R == 0:  # (an empty tensor has no address to hand over)
            return (values, sm) if sums else values
        with torch.cuda.device(self.device):
            L.check(self._lib.oth_ntuple_eval(self.board_size, R, ctypes.byref(self.params), _ptr(self.plan),
                                              self.plan_bytes, _ptr(w), self.weight_count, _ptr(bd), _ptr(mt),
                                              _ptr(values), _ptr(sm), _stream(self.device)), "oth_ntuple_eval")
        return (values, sm) if sums else values

    def update(self, boards, meta, targets, rate, rate_shift, mask=None):
        """One delta-rule step on the rows, in place on `weights`: with v the value of a
        row under the weights before the call, d = clamp(round((clamp(target, -32768,
        32768) - v) rate / 2^rate_shift), -2^30, 2^30) is added to every entry the row
        hits, once per hit, and to the bias.  Integer additions: the result is the same
        whatever the order.  mask (oth_ntuple_update_masked): a uint8 / bool tensor
        (R,), a row it leaves out gets delta 0 and adds nothing -- the rows stay where
        they are and nothing is read back to count them.  Returns the deltas, int32 (R,)."""
        R, bd, mt = self._rows(boards, meta)
        w = self._weights()
        tg = targets.to(device=self.device, dtype=torch.int32).contiguous()
        if tg.numel() != R:
            raise ValueError("expected %d targets, got %d" % (R, tg.numel()))
        mk = None
        if mask is not None:
            mk = mask.to(device=self.device).contiguous()
            mk = mk.view(torch.uint8) if mk.dtype == torch.bool else mk.to(torch.uint8)
            if mk.numel() != R:
                raise ValueError("expected a mask of %d rows, got %d" % (R, mk.numel()))
        deltas = torch.empty(R, dtype=torch.int32, device=self.device)
        if R == 0:
            return deltas
        with torch.cuda.device(self.device):
            if mk is None:
                L.check(self._lib.oth_ntuple_update(self.board_size, R, ctypes.byref(self.params), _ptr(self.plan),
                                                    self.plan_bytes, _ptr(w), self.weight_count, _ptr(bd), _ptr(mt),
                                                    _ptr(tg), int(rate), int(rate_shift), _ptr(deltas),
                                                    _stream(self.device)), "oth_ntuple_update")
            else:
                L.check(self._lib.oth_ntuple_update_masked(self.board_size, R, ctypes.byref(self.params),
                                                           _ptr(self.plan), self.plan_bytes, _ptr(w),
                                                           self.weight_count, _ptr(bd), _ptr(mt), _ptr(tg), _ptr(mk),
                                                           int(rate), int(rate_shift), _ptr(deltas),
                                                           _stream(self.device)), "oth_ntuple_update_masked")
        return deltas

    def td_play(self, env, n_plies, rate, rate_shift, explore=0.0, depth=1):
        """One TD(0) round in two calls and no host synchronisation: n_plies plies of
        self-play under this net on both sides (VecOthelloEnv.play_ntuple with td=True:
        an NTuplePlayer of `depth` that explores with probability `explore`), then one
        masked update over the n_plies * E rows with the rows' `learn` as the mask.
        The weights are frozen during the play launch: batch semantics, exact and
        order-independent.  Returns play_ntuple's result, the TDRows last."""
        key = (int(depth), float(explore))
        player = self._td_players.get(key)
        if player is None:
            player = self._td_players[key] = NTuplePlayer(self, depth=depth, explore=explore)
        res = env.play_ntuple(player, None, n_plies, td=True)
        rows = res[-1]
        R = rows.learn.numel()
        self.update(rows.boards.view(R, -1), rows.meta.view(R), rows.targets.view(R), rate, rate_shift,
                    mask=rows.learn.view(R))
        return res

    def rate_for(self, alpha, rows):
        """(rate, rate_shift) of a step `alpha` in value space for a batch of `rows`
        rows: a row's delta reaches its own sum through 8 T + 1 entries, so alpha = 1
        with rate / 2^rate_shift = 2^value_shift / ((8 T + 1) rows) closes a row's
        error if the rows shared no entry.  rate_shift is 24 -- lower where the rate
        would pass 2^24, higher (up to 40) where it would have fewer than 12 bits."""
        per = float(alpha) * 2.0 ** self.value_shift / ((8 * len(self.tuples) + 1) * int(rows))
        if not per > 0.0:
            return 0, 0
        shift = 24
        while shift > 0 and round(per * 2.0 ** shift) > L.OTH_NTUPLE_MAX_RATE:
            shift -= 1
        while shift < L.OTH_NTUPLE_MAX_RATE_SHIFT and per * 2.0 ** shift < 4096.0:
            shift += 1
        return min(int(round(per * 2.0 ** shift)), L.OTH_NTUPLE_MAX_RATE), shift

    def _check_env(self, env):
        if env.board_size != self.board_size:
            raise ValueError("the network is for %d x %d boards, the env has %d x %d" % (
                self.board_size, self.board_size, env.board_size, env.board_size))
        if torch.device(env.device) != self.device:
            raise ValueError("the network lives on %s, the env on %s" % (self.device, env.device))

    def __repr__(self):
        return "NTupleNet(<%d x %d, %d tuples, %d weights>, value_shift=%d)" % (
            self.board_size, self.board_size, len(self.tuples), self.weight_count, self.value_shift)


TDRows = collections.namedtuple("TDRows", "boards meta targets learn")
TDRows.__doc__ = """The TD(0) rows of VecOthelloEnv.play_ntuple(td=True) (struct oth_ntuple_td): boards int64
(n_plies, E, 2W) and meta int16 (n_plies, E), the row before each ply; targets int32 (n_plies, E), from
that row's mover's side; learn uint8 (n_plies, E), 1 where the ply was a finished search's move of a live
board -- every other row is zero."""


class NTuplePlayer(object):
    """An n-tuple network as a player (struct oth_ntuple_policy): the move of a board with
    e empty squares is oth_search_ntuple's `best` over `net` at depth e when e <=
    endgame_empties, else at `depth`; where the search runs over max_nodes (per root
    move) GreedyPolicy moves and the ply counts as a fallback.  Before the search, with
    probability `explore` (stored as round(65536 explore), a draw keyed by the env's
    seed, the board's global id and the ply) the ply explores: a uniform move of the
    stored possible moves, no fallback, no TD row.  Used by VecOthelloEnv.play_ntuple
    and as `opponent` of reset_vs / step_vs.  The net's weights are read as they are
    when a launch runs."""

    kind = "ntuple"

    def __init__(self, net, depth=1, endgame_empties=0, explore=0.0, terminal=64, max_nodes=1 << 22):
        if not isinstance(net, NTupleNet):
            raise TypeError("NTuplePlayer takes an NTupleNet")
        for name, v, lo, hi in (("depth", depth, 1, L.OTH_SEARCH_MAX_DEPTH), ("terminal", terminal, 1, 32767),
                                ("endgame_empties", endgame_empties, 0, L.OTH_SEARCH_MAX_DEPTH),
                                ("max_nodes", max_nodes, 1, 2 ** 32 - 1)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError("%s must be an integer" % name)
            if not lo <= int(v) <= hi:
                raise ValueError("%s must be in [%d, %d]" % (name, lo, hi))
        if not 0.0 <= float(explore) <= 1.0:
            raise ValueError("explore must be in [0, 1]")
        self.net = net
        self.depth, self.terminal = int(depth), int(terminal)
        self.endgame_empties, self.max_nodes = int(endgame_empties), int(max_nodes)
        self.explore = int(round(L.OTH_NTUPLE_EXPLORE_ONE * float(explore)))
        self._pol = None

    def _policy(self, env):
        """The struct for a call on env, with the net's weights as they are now (kept alive here)."""
        net = self.net
        net._check_env(env)
        w = net._weights()
        pol = L.OthNtuplePolicy()
        ctypes.memmove(ctypes.byref(pol.params), ctypes.byref(net.params), ctypes.sizeof(L.OthNtupleParams))
        pol.plan, pol.plan_bytes = net.plan.data_ptr(), net.plan_bytes
        pol.weights, pol.weight_count = w.data_ptr(), net.weight_count
        pol.depth, pol.terminal_weight, pol.endgame_empties = self.depth, self.terminal, self.endgame_empties
        pol.explore, pol.max_nodes = self.explore, self.max_nodes
        self._pol = (pol, w)
        return pol

    def __repr__(self):
        return "NTuplePlayer(%r, depth=%d, endgame_empties=%d, explore=%d/65536, terminal=%d, max_nodes=%d)" % (
            self.net, self.depth, self.endgame_empties, self.explore, self.terminal, self.max_nodes)


class ntuple_evaluator(object):
    """An NTupleNet as an evaluator of puct_search / puct_play: zero logits (a uniform
    prior over the legal squares) and the net's value of the leaf as a float, v /
    32768 -- which puct_quantize turns back into exactly the integer v."""

    def __init__(self, net):
        self.net = net

    def __call__(self, leaves):
        v = self.net.evaluate(leaves.boards, leaves.meta)
        nn = self.net.board_size * self.net.board_size
        return torch.zeros(v.numel(), nn, device=v.device), v.to(torch.float32) / float(L.OTH_PUCT_VALUE_ONE)
