"""VecOthelloEnv -- E Othello boards resident in HBM, stepped by HIP kernels.

The batched form of the reference's OthelloBaseEnv (othello.py:217-501): one
handle of the C ABI (include/othello_mi355x.h) owns E boards on one GPU; every
method enqueues kernels on the current torch stream and returns torch tensors
that stay on the device.  It replaces the reference's CPU "vector env" of one
process per board (envs.py:7-287) for the hot path; torch here is only device
memory, streams and the collective for the W/D/L tally.
"""
import collections
import contextlib
import ctypes

import torch

from . import _lib as L
from .masked import _rows

_OBS_LAYOUTS = {"board": L.OTH_OBS_BOARD, "board_legal": L.OTH_OBS_BOARD_LEGAL,
                "make_state": L.OTH_OBS_MAKE_STATE, "absolute": L.OTH_OBS_ABSOLUTE, "legal": L.OTH_OBS_LEGAL}
_OBS_PLANES = {L.OTH_OBS_BOARD: 1, L.OTH_OBS_BOARD_LEGAL: 2, L.OTH_OBS_MAKE_STATE: 4, L.OTH_OBS_ABSOLUTE: 1,
               L.OTH_OBS_LEGAL: 1}
_ONE_PLANE = (L.OTH_OBS_BOARD, L.OTH_OBS_ABSOLUTE, L.OTH_OBS_LEGAL)
_DTYPES = {torch.int8: L.OTH_I8, torch.int32: L.OTH_I32, torch.int64: L.OTH_I64,
           torch.float32: L.OTH_F32, torch.float64: L.OTH_F64, torch.bfloat16: L.OTH_BF16}
_POLICIES = {"random": L.OTH_POLICY_RANDOM, "greedy": L.OTH_POLICY_GREEDY}
_POLICIES.update({"maximin%d" % d: L.OTH_POLICY_MAXIMIN(d) for d in range(1, L.OTH_MAXIMIN_MAX_DEPTH + 1)})

BLACK_DISK, NO_DISK, WHITE_DISK = -1, 0, 1  # othello.py:10-12

# playouts(seed=None) keys its draws with the env's seed XOR this constant (the 64-bit golden ratio),
# so playouts never share a Philox key with the env's own play
PLAYOUT_SEED_XOR = 0x9E3779B97F4A7C15


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def nwords(n):
    return (n * n + 63) // 64


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# the leaves of a network-guided search (VecOthelloEnv.puct_begin / puct_advance)
PuctLeaves = collections.namedtuple("PuctLeaves", ("kind", "boards", "meta", "legal", "obs"))
# one move of self-play on the search's tree (VecOthelloEnv.puct_play)
PuctPlay = collections.namedtuple("PuctPlay", ("actions", "visits", "rewards", "dones", "kept"))
# a minibatch of the replay store (VecOthelloEnv.replay_gather / replay_sample)
ReplayBatch = collections.namedtuple("ReplayBatch", ("state", "boards", "meta", "legal", "visits", "outcome", "obs",
                                                     "rows", "sym"))


def puct_quantize(logits, leaf_legal, values):
    """The integers oth_puct_advance takes, from a network's floats: priors int32
    (E, N*N) = round(65535 p), p the softmax of `logits` (E, N*N) over the leaf's
    legal squares (`leaf_legal`: PuctLeaves.legal, int64 (E, W)) in float32 on the
    device, 0 elsewhere (and on a leaf without a legal square); values int32 (E,) =
    round(32768 clamp(v, -1, 1)), v the value for the leaf's side to move.

    This is the only place of the search where floats appear: the search is exact
    *given* these integers, which is what its tests pin; how a network's floats
    round is the caller's business."""
    E = logits.shape[0]
    lg = logits.reshape(E, -1).to(torch.float32)
    nn = lg.shape[1]
    a = torch.arange(nn, device=lg.device)
    mask = ((leaf_legal.to(lg.device).view(E, -1)[:, a // 64] >> (a % 64)) & 1).bool()
    p = torch.softmax(lg.masked_fill(~mask, float("-inf")), dim=1)
    p = torch.where(mask, p, torch.zeros_like(p))  # (a row without a legal square: nan -> 0)
    priors = torch.round(p * float(L.OTH_PUCT_PRIOR_MAX)).to(torch.int32)
    v = values.reshape(E).to(device=lg.device, dtype=torch.float32).clamp(-1.0, 1.0)
    return priors, torch.round(v * float(L.OTH_PUCT_VALUE_ONE)).to(torch.int32)


def _puct_evaluate(evaluate, leaves):
    """What puct_search, puct_play and the batch loop give to the advance: evaluate's
    (logits, values) quantised by puct_quantize, or, from an evaluator whose
    `quantized` attribute is true (net.DeviceNet), its (priors, values) as they are."""
    out, values = evaluate(leaves)
    if getattr(evaluate, "quantized", False):
        return out, values
    return puct_quantize(out, leaves.legal, values)


def _leaves_board_size(leaves):
    if leaves.obs is None:
        raise ValueError("this evaluator takes the board size from leaves.obs: begin the search with a layout")
    return int(leaves.obs.shape[-1])


def uniform_evaluator(leaves):
    """The evaluator that knows nothing: zero logits (a uniform prior over the legal
    squares) and value 0.  With it the search is a breadth-first tree whose only
    values are the game ends it reaches."""
    n, E = _leaves_board_size(leaves), leaves.kind.shape[0]
    dev = leaves.kind.device
    return torch.zeros(E, n * n, device=dev), torch.zeros(E, device=dev)


class playout_evaluator(object):
    """An evaluator without a network: the value of a leaf is (wins - losses) / R of
    R random games from it, played on the device by a private second VecOthelloEnv
    that is loaded with the leaves (set_state) -- the leaf evaluation of mcts(),
    through the evaluator interface; the logits are zero.  It shows how an
    evaluator plugs in; a learner puts its network here.  Playouts are keyed by
    `seed` and a call counter, so a search repeats."""

    def __init__(self, n_playouts=8, seed=0):
        self.n_playouts, self.seed, self.counter = int(n_playouts), int(seed), 0
        self._env = None

    def __call__(self, leaves):
        n, E = _leaves_board_size(leaves), leaves.kind.shape[0]
        env = self._env
        if env is None or env.num_envs != E or env.board_size != n or env.device != leaves.kind.device:
            if env is not None:
                env.close()
            env = self._env = VecOthelloEnv(E, board_size=n, device=leaves.kind.device)
        env.set_state(leaves.boards, leaves.meta, leaves.legal)
        wdl = env.playouts(self.n_playouts, seed=self.seed, counter=self.counter)
        self.counter += 1
        values = (wdl[:, 0] - wdl[:, 2]).to(torch.float32) / float(self.n_playouts)
        return torch.zeros(E, n * n, device=values.device), values


class VecOthelloEnv(object):
    """E independent boards of one size on one GPU.

    Args mirror OthelloBaseEnv / SimpleOthelloEnv (othello.py:26-33, 222-227);
    the batched extras are `auto_reset` (reset a board right after its terminal
    ply), `seed` / `env_id_base` (Philox key and this shard's first global env
    id) and `device`.
    """

    def __init__(self, num_envs, board_size=8, sudden_death_on_invalid_move=True,
                 num_disk_as_reward=False, possible_actions_in_obs=False, auto_reset=False,
                 initial_rand_steps=0, seed=0, env_id_base=0, device=None, lib=None):
        self._lib = lib if lib is not None else L.load()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:  # "cuda" -> the current device, by index
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_envs = int(num_envs)
        self.board_size = max(4, int(board_size))  # othello.py:230
        self.words = nwords(self.board_size)
        self.sudden_death_on_invalid_move = bool(sudden_death_on_invalid_move)
        self.num_disk_as_reward = bool(num_disk_as_reward)
        self.possible_actions_in_obs = bool(possible_actions_in_obs)
        self.auto_reset = bool(auto_reset)
        self.initial_rand_steps = int(initial_rand_steps)
        self.seed = int(seed)
        self.env_id_base = int(env_id_base)
        flags = ((L.OTH_SUDDEN_DEATH if self.sudden_death_on_invalid_move else 0) |
                 (L.OTH_DISK_REWARD if self.num_disk_as_reward else 0) |
                 (L.OTH_AUTO_RESET if self.auto_reset else 0))
        self.flags = flags
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self._lib.oth_create(self.num_envs, self.board_size, flags, self.seed & (2 ** 64 - 1),
                                         self.env_id_base, self.initial_rand_steps, self.device.index,
                                         ctypes.byref(h)), "oth_create")
        self._h = h
        self._hv = h.value  # the handle as an int: the per-step ctypes calls take it as is
        self._dev_index = self.device.index
        self._step_fn = self._lib.oth_step
        self._step_obs_fn = self._lib.oth_step_observe
        self._bview = None  # (dones tensor, its bool view): step()'s view of caller-given dones, cached
        self._okbufs = None  # (rewards, dones) tensors step() has checked
        self._okobs = None  # (obs tensor, layout) step() / sample_step() have checked
        self._sample_calls = 0  # Philox counter of sample_actions
        self._playout_calls = 0  # `counter` of the next playouts() call that gives none
        self._pick_calls = 0  # `counter` of the next sampling puct_pick() call that gives none
        self._noise_calls = 0  # `counter` of the next puct_noise() call that gives none
        self._mcts_ws = None  # mcts()'s workspace: a uint8 tensor, regrown only when too small
        self._puct_ws = None  # the puct_* search's workspace, its own: mcts() would overwrite a search in progress
        self._puct = None  # the search in progress: (params, the C leaves struct, PuctLeaves)
        self._puct_k = 0  # its leaves per board in the batch calls; 0: the plain calls began it
        self._replay_ws = None  # the replay store's workspace, regrown only when too small
        self._replay = None  # the store in use: (horizon, max_batch)
        self._replay_calls = 0  # `counter` of the next replay_sample() call that gives none
        self._region_resets = None  # resets inside an open graph region (None: no region)

    # ------------------------------------------------------------------ utils
    def _stream(self):
        if _RAW_STREAM is not None:  # the current stream's handle without building a Stream object
            return ctypes.c_void_p(_RAW_STREAM(self.device.index))
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.oth_destroy(self._h)
            self._h = None
            self._hv = None  # a later step() passes NULL: OTH_EINVAL, not a freed handle

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _i32(self, *shape):
        return torch.empty(*shape, dtype=torch.int32, device=self.device)

    def _u8(self, *shape):
        return torch.empty(*shape, dtype=torch.uint8, device=self.device)

    def _out(self, given, dtype, name):
        """An (E,) output: a new tensor for None / True, nothing for False, or the
        caller's tensor (checked) to be written in place."""
        if given is None or given is True:
            return torch.empty(self.num_envs, dtype=dtype, device=self.device)
        if given is False:
            return None
        if given.dtype != dtype or given.numel() != self.num_envs or not given.is_contiguous() or \
                given.device != self.device:
            raise ValueError("%s must be a contiguous %s tensor of %d elements on %s" %
                             (name, dtype, self.num_envs, self.device))
        return given

    @property
    def ply_counter(self):
        return int(self._lib.oth_ply_counter(self._h))

    @ply_counter.setter
    def ply_counter(self, v):
        if getattr(self, "_region_resets", None) is not None:
            raise RuntimeError("cannot set the ply counter inside a graph region")
        L.check(self._lib.oth_set_ply_counter(self._h, int(v)), "oth_set_ply_counter")

    # ---------------------------------------------------------------- the API
    def reset(self, mask=None):
        """OthelloBaseEnv.reset (othello.py:265-271) for every board (or where mask)."""
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        if getattr(self, "_region_resets", None) is not None:
            self._region_resets += 1
        L.check(self._lib.oth_reset(self._h, _ptr(m), self._stream()), "oth_reset")
        return self.get_observation()

    def step(self, actions, rewards=None, dones=None, observe=True, obs=None, obs_layout=None,
             obs_dtype=torch.int64):
        """OthelloBaseEnv.step (othello.py:412-462) on every board.

        actions: int tensor (E,).  rewards / dones: optional int32 / uint8 (or
        bool) (E,) tensors on this device, written in place (the loop form: no
        allocation per step; checked once per tensor).  Returns (obs, rewards
        int32 (E,), dones bool (E,), None).  With observe (the default) obs is the
        step's get_observation() (othello.py:462) -- or `obs_layout` ('board',
        'board_legal', 'make_state', 'absolute', 'legal') -- written by the same
        launch that stepped the boards (oth_step_observe), into `obs` if given (its
        dtype decides the element type) or a new `obs_dtype` tensor; None when
        observe=False.  The host path is one ctypes call: an int32 contiguous
        action tensor on this device is passed as is."""
        a = actions
        if a.dtype is not torch.int32 or not a.is_contiguous() or a.device != self.device:
            a = a.to(device=self.device, dtype=torch.int32).contiguous()
        if a.numel() != self.num_envs:
            raise ValueError("expected %d actions, got %d" % (self.num_envs, a.numel()))
        r = rewards if rewards is not None else self._i32(self.num_envs)
        d = dones if dones is not None else self._u8(self.num_envs)
        ok = self._okbufs
        # caller-given buffers: checked once each, and again if resize_() / set_() moved or shrank them
        if ok is None or ok[0] is not r or ok[1] is not d or ok[2] != (r.data_ptr(), d.data_ptr(), r.numel(),
                                                                      d.numel()):
            self._check_out(r, (torch.int32,), "rewards")
            self._check_out(d, (torch.uint8, torch.bool), "dones")
            self._okbufs = (r, d, (r.data_ptr(), d.data_ptr(), r.numel(), d.numel()))
        st = _RAW_STREAM(self._dev_index) if _RAW_STREAM is not None else self._stream()
        if observe:
            lay, o = self._obs_out(obs_layout, obs_dtype, obs)
            rc = self._step_obs_fn(self._hv, a.data_ptr(), r.data_ptr(), d.data_ptr(), lay, _DTYPES[o.dtype],
                                   o.data_ptr(), st)
            if rc:
                L.check(rc, "oth_step_observe")
        else:
            o = None
            rc = self._step_fn(self._hv, a.data_ptr(), r.data_ptr(), d.data_ptr(), st)
            if rc:
                L.check(rc, "oth_step")
        bv = self._bview
        if bv is None or bv[0] is not d:  # 0/1 bytes: a view, not a conversion kernel
            bv = self._bview = (d, d if d.dtype is torch.bool else d.view(torch.bool))
        return o, r, bv[1], None

    def _check_out(self, t, dtypes, name):
        """A caller-given (E,) output the kernels write: on this device, contiguous,
        E elements of one of `dtypes` -- else ValueError before any launch."""
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.device != self.device or \
                not t.is_contiguous() or t.numel() != self.num_envs:
            raise ValueError("%s must be a contiguous %s tensor of %d elements on %s" %
                             (name, " or ".join(str(x) for x in dtypes), self.num_envs, self.device))

    def _obs_shape(self, lay):
        n = self.board_size
        return (self.num_envs, n, n) if lay in _ONE_PLANE else (self.num_envs, _OBS_PLANES[lay], n, n)

    def _obs_out(self, layout, dtype, out):
        """(layout id, output tensor) of a fused observation: get_observation()'s
        layout unless given; `out` checked once per tensor, or a new tensor."""
        if layout is None:
            lay = L.OTH_OBS_BOARD_LEGAL if self.possible_actions_in_obs else L.OTH_OBS_BOARD
        else:
            lay = _OBS_LAYOUTS[layout] if isinstance(layout, str) else int(layout)
            if lay not in _OBS_PLANES:
                raise ValueError("unknown observation layout %r" % (layout,))
        if out is None:
            if dtype not in _DTYPES:
                raise ValueError("observation dtype must be one of %s" % list(_DTYPES))
            return lay, torch.empty(self._obs_shape(lay), dtype=dtype, device=self.device)
        ok = self._okobs
        if ok is None or ok[0] is not out or ok[1] != lay or ok[2] != (out.data_ptr(), out.numel(), out.dtype):
            shape = self._obs_shape(lay)
            if out.dtype not in _DTYPES or out.device != self.device or not out.is_contiguous() or \
                    out.numel() != _numel(shape):
                raise ValueError("obs must be a contiguous tensor of %s elements (shape %s) of one of %s on %s" %
                                 (_numel(shape), shape, list(_DTYPES), self.device))
            self._okobs = (out, lay, (out.data_ptr(), out.numel(), out.dtype))
        return lay, out

    def step_policy(self, policy="random", n_plies=1, actions=None, rewards=None, dones=None, record=True):
        """n_plies plies where every board's mover plays `policy` on the device
        (RandomPolicy simple_policies.py:37-41, GreedyPolicy :69-92, MaxiMinPolicy
        :98-163 as 'maximin1'..'maximin10').

        Returns (actions, rewards, dones) of shape (n_plies, E) (None if not recorded)."""
        pol = _POLICIES[policy] if isinstance(policy, str) else int(policy)
        if record:
            actions = actions if actions is not None else self._i32(n_plies, self.num_envs)
            rewards = rewards if rewards is not None else self._i32(n_plies, self.num_envs)
            dones = dones if dones is not None else self._u8(n_plies, self.num_envs)
        L.check(self._lib.oth_step_policy(self._h, pol, int(n_plies), _ptr(actions), _ptr(rewards),
                                          _ptr(dones), self._stream()), "oth_step_policy")
        return actions, rewards, dones

    def play_search(self, black, white=None, n_plies=1, record=True, fallbacks=False):
        """n_plies plies where every board's mover plays its colour's searched move
        (oth_play_search): step_policy with the policy's move replaced by the
        SearchConfig's -- `black` for black's plies, `white` (None: `black`) for
        white's -- in one launch that never synchronises the host.  Random-opening
        plies, terminated boards, auto-reset, the tallies and the ply counter are
        step_policy's.

        Returns (actions, rewards, dones) of shape (n_plies, E) (None if not
        recorded), and with fallbacks=True a uint8 (n_plies, E) tensor that is 1
        where the ply's search ran over max_nodes and GreedyPolicy moved."""
        if not isinstance(black, SearchConfig) or not (white is None or isinstance(white, SearchConfig)):
            raise TypeError("play_search takes SearchConfig objects")
        n_plies = int(n_plies)
        if n_plies < 1:
            raise ValueError("n_plies must be >= 1")
        pb = black._policy(self)
        pw = pb if white is None or white is black else white._policy(self)
        a = r = d = None
        if record:
            a, r, d = self._i32(n_plies, self.num_envs), self._i32(n_plies, self.num_envs), self._u8(n_plies, self.num_envs)
        f = self._u8(n_plies, self.num_envs) if fallbacks else None
        L.check(self._lib.oth_play_search(self._h, ctypes.addressof(pb), ctypes.addressof(pw), n_plies, _ptr(a),
                                          _ptr(r), _ptr(d), _ptr(f), self._stream()), "oth_play_search")
        return (a, r, d, f) if fallbacks else (a, r, d)

    def play_net(self, black, white=None, n_plies=1, record=True):
        """n_plies plies where every board's mover plays its colour's network's move
        (oth_play_net): step_policy with the policy's move replaced by the
        NetPlayer's -- `black` for black's plies, `white` (None: `black`) for white's
        -- in one launch that never synchronises the host: the argmax of the logits
        over the stored legal squares, or a draw from the priors while the board has
        fewer than the player's sample_discs discs.  The two networks must have the
        same width.  With conv players (NetPlayer of a DeviceConvNet) the call is
        oth_play_cnet: the two must have the same channel count, and an MLP on one
        side with a conv net on the other is a ValueError.  Random-opening plies, terminated boards, auto-reset, the tallies
        and the ply counter are step_policy's.

        Returns (actions, rewards, dones) of shape (n_plies, E) (None if not
        recorded)."""
        from .net import NetPlayer
        if not isinstance(black, NetPlayer) or not (white is None or isinstance(white, NetPlayer)):
            raise TypeError("play_net takes NetPlayer objects")
        n_plies = int(n_plies)
        if n_plies < 1:
            raise ValueError("n_plies must be >= 1")
        if white is not None and white.kind != black.kind:
            raise ValueError("play_net takes two networks of one kind: an MLP against a conv net is not supported")
        conv = black.kind == "conv"
        if conv and white is not None and white.net.channels != black.net.channels:
            raise ValueError("the two conv nets of play_net must have the same channels (%d and %d)" % (
                black.net.channels, white.net.channels))
        pb = black._policy(self)
        pw = pb if white is None or white is black else white._policy(self)
        a = r = d = None
        if record:
            a, r, d = self._i32(n_plies, self.num_envs), self._i32(n_plies, self.num_envs), self._u8(n_plies, self.num_envs)
        call, what = (self._lib.oth_play_cnet, "oth_play_cnet") if conv else (self._lib.oth_play_net, "oth_play_net")
        L.check(call(self._h, ctypes.addressof(pb), ctypes.addressof(pw), n_plies, _ptr(a), _ptr(r), _ptr(d),
                     self._stream()), what)
        return a, r, d

    def play_ntuple(self, black, white=None, n_plies=1, record=True, fallbacks=False, td=False):
        """n_plies plies where every board's mover plays its colour's n-tuple player's
        move (oth_play_ntuple): play_search with the move replaced by the
        NTuplePlayer's -- `black` for black's plies, `white` (None: `black`) for
        white's; the two may differ in everything -- in one launch that never
        synchronises the host: an exploring ply's uniform move, else the alpha-beta's
        best move over the net, GreedyPolicy's where the search ran over max_nodes.
        Random-opening plies, terminated boards, auto-reset, the tallies and the ply
        counter are step_policy's.

        Returns play_search's result -- (actions, rewards, dones) of shape (n_plies, E)
        (None if not recorded), with fallbacks=True a uint8 (n_plies, E) tensor -- and
        with td=True an ntuple.TDRows last: the TD(0) rows of the plies from the same
        launch, what NTupleNet.update takes with `learn` as its mask."""
        from .ntuple import NTuplePlayer, TDRows
        if not isinstance(black, NTuplePlayer) or not (white is None or isinstance(white, NTuplePlayer)):
            raise TypeError("play_ntuple takes NTuplePlayer objects")
        n_plies = int(n_plies)
        if n_plies < 1:
            raise ValueError("n_plies must be >= 1")
        pb = black._policy(self)
        pw = pb if white is None or white is black else white._policy(self)
        E = self.num_envs
        a = r = d = None
        if record:
            a, r, d = self._i32(n_plies, E), self._i32(n_plies, E), self._u8(n_plies, E)
        f = self._u8(n_plies, E) if fallbacks else None
        rows = tdp = None
        if td:
            rows = TDRows(torch.empty(n_plies, E, 2 * self.words, dtype=torch.int64, device=self.device),
                          torch.empty(n_plies, E, dtype=torch.int16, device=self.device), self._i32(n_plies, E),
                          self._u8(n_plies, E))
            tds = L.OthNtupleTd(*[t.data_ptr() for t in rows])
            tdp = ctypes.addressof(tds)
        L.check(self._lib.oth_play_ntuple(self._h, ctypes.addressof(pb), ctypes.addressof(pw), n_plies, _ptr(a),
                                          _ptr(r), _ptr(d), _ptr(f), tdp, self._stream()), "oth_play_ntuple")
        return (a, r, d) + ((f,) if fallbacks else ()) + ((rows,) if td else ())

    # ------------------------------------------- OthelloEnv semantics on device
    def _protagonist(self, protagonist):
        if protagonist is None:
            return getattr(self, "_prot", None)
        if isinstance(protagonist, int):
            protagonist = torch.full((self.num_envs,), protagonist, dtype=torch.int8)
        t = protagonist.to(device=self.device, dtype=torch.int8).contiguous()
        if t.numel() != self.num_envs:
            raise ValueError("protagonist needs one colour per board")
        self._prot = t
        return t

    def reset_vs(self, opponent="random", protagonist=None, mask=None):
        """OthelloEnv.reset (othello.py:151-174) for every board: reset, then the
        embedded opponent (`opponent` = 'random' | 'greedy', played on the device)
        replies until the protagonist (+1 white, the reference default, or -1
        black; int or per-board tensor) is to move.  `opponent` may be a
        SearchConfig: the opponent then plays its searched move (oth_reset_vs_search);
        or a NetPlayer: it plays its network's move (oth_reset_vs_net, or
        oth_reset_vs_cnet for a conv net); or an NTuplePlayer: its n-tuple player's
        move (oth_reset_vs_ntuple)."""
        from .net import NetPlayer
        prot = self._protagonist(protagonist)
        m = None if mask is None else mask.to(device=self.device, dtype=torch.uint8).contiguous()
        if isinstance(opponent, NetPlayer):
            call, what = ((self._lib.oth_reset_vs_cnet, "oth_reset_vs_cnet") if opponent.kind == "conv" else
                          (self._lib.oth_reset_vs_net, "oth_reset_vs_net"))
            L.check(call(self._h, ctypes.addressof(opponent._policy(self)), _ptr(prot), _ptr(m), self._stream()), what)
            return self.get_observation()
        if isinstance(opponent, SearchConfig):
            L.check(self._lib.oth_reset_vs_search(self._h, ctypes.addressof(opponent._policy(self)), _ptr(prot),
                                                  _ptr(m), self._stream()), "oth_reset_vs_search")
            return self.get_observation()
        if getattr(opponent, "kind", None) == "ntuple":  # an ntuple.NTuplePlayer
            L.check(self._lib.oth_reset_vs_ntuple(self._h, ctypes.addressof(opponent._policy(self)), _ptr(prot),
                                                  _ptr(m), self._stream()), "oth_reset_vs_ntuple")
            return self.get_observation()
        L.check(self._lib.oth_reset_vs(self._h, _POLICIES[opponent], _ptr(prot), _ptr(m), self._stream()),
                "oth_reset_vs")
        return self.get_observation()

    def step_vs(self, actions, opponent="random", protagonist=None, observe=True, obs=None, obs_layout=None,
                obs_dtype=torch.int64, fallbacks=False):
        """OthelloEnv.step (othello.py:176-200) for every board: the protagonist
        plays `actions`, the device opponent replies until the protagonist is to
        move again.  Returns (obs, rewards (protagonist's view, negated after an
        opponent ply ended the game), dones bool, plies applied per board).  The
        observation (get_observation's layout unless `obs_layout`; into `obs` if
        given) comes from the same launch (oth_step_vs_observe).

        `opponent` may be a SearchConfig: the opponent plays its searched move
        (oth_step_vs_search, one launch, no host round trip per reply), the
        observation comes from an observe launch after it, and with fallbacks=True
        a fifth result counts, per board, the opponent's plies of this call whose
        search ran over max_nodes and were played by GreedyPolicy (int32 (E,)).
        An NTuplePlayer opponent (oth_step_vs_ntuple) goes the same way, fallbacks
        included.

        `opponent` may be a NetPlayer: the opponent plays its network's move
        (oth_step_vs_net, or oth_step_vs_cnet for a conv net: one launch, no host
        round trip per reply) and the
        observation comes from an observe launch after it; fallbacks=True raises."""
        from .net import NetPlayer
        prot = self._protagonist(protagonist)
        a = actions.to(device=self.device, dtype=torch.int32).contiguous()
        if a.numel() != self.num_envs:
            raise ValueError("expected %d actions, got %d" % (self.num_envs, a.numel()))
        r, d, n = self._i32(self.num_envs), self._u8(self.num_envs), self._i32(self.num_envs)
        if isinstance(opponent, NetPlayer):
            if fallbacks:
                raise ValueError("fallbacks are a search opponent's: a NetPlayer has none")
            o = None
            if observe:
                lay, o = self._obs_out(obs_layout, obs_dtype, obs)
            call, what = ((self._lib.oth_step_vs_cnet, "oth_step_vs_cnet") if opponent.kind == "conv" else
                          (self._lib.oth_step_vs_net, "oth_step_vs_net"))
            L.check(call(self._h, ctypes.addressof(opponent._policy(self)), _ptr(a), _ptr(prot), _ptr(r), _ptr(d),
                         _ptr(n), self._stream()), what)
            if observe:
                L.check(self._lib.oth_observe(self._h, lay, _DTYPES[o.dtype], _ptr(o), self._stream()), "oth_observe")
            return o, r, d.view(torch.bool), n
        ntuple = getattr(opponent, "kind", None) == "ntuple"  # an ntuple.NTuplePlayer
        if isinstance(opponent, SearchConfig) or ntuple:
            f = self._i32(self.num_envs) if fallbacks else None
            o = None
            if observe:
                lay, o = self._obs_out(obs_layout, obs_dtype, obs)
            call, what = ((self._lib.oth_step_vs_ntuple, "oth_step_vs_ntuple") if ntuple else
                          (self._lib.oth_step_vs_search, "oth_step_vs_search"))
            L.check(call(self._h, ctypes.addressof(opponent._policy(self)), _ptr(a), _ptr(prot), _ptr(r), _ptr(d),
                         _ptr(n), _ptr(f), self._stream()), what)
            if observe:
                L.check(self._lib.oth_observe(self._h, lay, _DTYPES[o.dtype], _ptr(o), self._stream()), "oth_observe")
            res = (o, r, d.view(torch.bool), n)
            return res + (f,) if fallbacks else res
        if fallbacks:
            raise ValueError("fallbacks are a search opponent's: pass a SearchConfig as opponent")
        if observe:
            lay, o = self._obs_out(obs_layout, obs_dtype, obs)
            L.check(self._lib.oth_step_vs_observe(self._h, _POLICIES[opponent], _ptr(a), _ptr(prot), _ptr(r),
                                                  _ptr(d), _ptr(n), lay, _DTYPES[o.dtype], _ptr(o), self._stream()),
                    "oth_step_vs_observe")
        else:
            o = None
            L.check(self._lib.oth_step_vs(self._h, _POLICIES[opponent], _ptr(a), _ptr(prot), _ptr(r), _ptr(d),
                                          _ptr(n), self._stream()), "oth_step_vs")
        return o, r, d.view(torch.bool), n

    def legal_mask(self):
        """possible_moves of every board as (E, W) int64 bit masks (bit a = square a)."""
        out = torch.empty(self.num_envs, self.words, dtype=torch.int64, device=self.device)
        L.check(self._lib.oth_legal(self._h, _ptr(out), self._stream()), "oth_legal")
        return out

    def legal_actions(self):
        """possible_moves as a bool (E, N*N) tensor: the OTH_OBS_LEGAL plane in int8,
        viewed as bool (one kernel writing E*N*N bytes, no conversion)."""
        o = self.observe("legal", torch.int8)
        return o.view(torch.bool).reshape(self.num_envs, -1)

    def greedy_actions(self):
        """GreedyPolicy.get_action (simple_policies.py:69-92) for every board."""
        return self.policy_actions("greedy")

    def policy_actions(self, policy="greedy"):
        """The move of a scripted policy ('greedy', 'maximin<d>'; simple_policies.py:57-163)
        for the side to move on every board.

        MaxiMin accepts any depth, as the reference does (:101-103).  Every search
        level places a disc, so a search deeper than a board's empty squares is the
        search of depth = its empty squares (the board is full, hence terminal, at
        that level either way, :117-126).  Beyond OTH_MAXIMIN_MAX_DEPTH the call
        therefore runs at the largest empty-square count of the batch's live
        boards when that is at most OTH_MAXIMIN_MAX_DEPTH (bit-identical), and
        raises otherwise.  Depth <= 0 searches nothing: the reference's search
        stops at the root and returns no move (:117-126), so every board gets -1.
        Calls the C ABI estimates above OTH_MAXIMIN_LEAF_BUDGET leaves (bounded by
        each board's empty squares) raise OthelloLibError."""
        if isinstance(policy, str) and policy.startswith("maximin") and policy not in _POLICIES:
            try:
                d = int(policy[len("maximin"):])
            except ValueError:
                raise ValueError("unknown policy %r: 'greedy' or 'maximin<depth>'" % (policy,)) from None
            if d <= 0:
                return torch.full((self.num_envs,), -1, dtype=torch.int32, device=self.device)
            # (a terminated board's search returns no move at the root, whatever the depth)
            live = ~self.terminated()
            left = self.board_size ** 2 - self.count_disks().sum(1)
            empties = int(left[live].max()) if bool(live.any()) else 0
            if empties > L.OTH_MAXIMIN_MAX_DEPTH:
                raise ValueError("maximin%d: a board has %d empty squares; the device search covers depths up to "
                                 "%d, or any depth once every board has at most %d empty squares"
                                 % (d, empties, L.OTH_MAXIMIN_MAX_DEPTH, L.OTH_MAXIMIN_MAX_DEPTH))
            policy = "maximin%d" % max(1, min(d, empties))
        if isinstance(policy, str) and policy not in _POLICIES:
            raise ValueError("unknown policy %r: 'greedy' or 'maximin<depth>'" % (policy,))
        out = self._i32(self.num_envs)
        L.check(self._lib.oth_policy_actions(self._h, _POLICIES[policy], _ptr(out), self._stream()),
                "oth_policy_actions")
        return out

    def observe(self, layout="board", dtype=torch.int64, out=None):
        lay = _OBS_LAYOUTS[layout] if isinstance(layout, str) else int(layout)
        planes = _OBS_PLANES[lay]
        n = self.board_size
        shape = (self.num_envs, n, n) if lay in _ONE_PLANE else (self.num_envs, planes, n, n)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=self.device)
        L.check(self._lib.oth_observe(self._h, lay, _DTYPES[out.dtype], _ptr(out), self._stream()),
                "oth_observe")
        return out

    def get_observation(self, dtype=torch.int64):
        """get_observation (othello.py:363-378): mover-perspective board, plus the
        possible-moves plane when possible_actions_in_obs."""
        return self.observe("board_legal" if self.possible_actions_in_obs else "board", dtype)

    def make_state(self, dtype=torch.float32):
        """util.make_state (util.py:48-74) for every board: (E, 4, N, N)."""
        return self.observe("make_state", dtype)

    def count_disks(self):
        """count_disks (othello.py:468-471): int32 (E, 2) = (white_cnt, black_cnt)."""
        out = self._i32(self.num_envs, 2)
        L.check(self._lib.oth_count_disks(self._h, _ptr(out), self._stream()), "oth_count_disks")
        return out

    def set_player_turn(self, turn, mask=None):
        """set_player_turn (othello.py:464-466): set the turn and recompute possible_moves."""
        m = None if mask is None else mask.to(device=self.device, dtype=torch.uint8).contiguous()
        L.check(self._lib.oth_set_player_turn(self._h, int(turn), _ptr(m), self._stream()),
                "oth_set_player_turn")

    def get_state(self):
        """(boards (E, 2W) int64, meta (E,) int16, legal (E, W) int64) device copies
        in the exchange format of include/othello_mi355x.h."""
        b = torch.empty(self.num_envs, 2 * self.words, dtype=torch.int64, device=self.device)
        m = torch.empty(self.num_envs, dtype=torch.int16, device=self.device)
        lg = torch.empty(self.num_envs, self.words, dtype=torch.int64, device=self.device)
        L.check(self._lib.oth_get_state(self._h, _ptr(b), _ptr(m), _ptr(lg), self._stream()), "oth_get_state")
        return b, m, lg

    def set_state(self, boards=None, meta=None, legal=None):
        def dev(t, dt):
            return None if t is None else t.to(device=self.device).contiguous().view(dt)
        b, m, lg = dev(boards, torch.int64), dev(meta, torch.int16), dev(legal, torch.int64)
        for t, per in ((b, 2 * self.words), (m, 1), (lg, self.words)):
            if t is not None and t.numel() != self.num_envs * per:
                raise ValueError("state tensor has %d elements, expected %d" % (t.numel(), self.num_envs * per))
        L.check(self._lib.oth_set_state(self._h, _ptr(b), _ptr(m), _ptr(lg), self._stream()), "oth_set_state")
        # keep the sources alive until the async copies ran
        torch.cuda.current_stream(self.device).synchronize()

    def counts(self, reset=False):
        """{black wins, draws, white wins} of games finished since the last reset (int64 (3,))."""
        out = torch.empty(3, dtype=torch.int64, device=self.device)
        L.check(self._lib.oth_counts(self._h, _ptr(out), int(bool(reset)), self._stream()), "oth_counts")
        return out

    def counts_vs(self, reset=False):
        """{protagonist wins, draws, protagonist losses} of games finished by
        step_vs (run.py:100-130's count, the README's table) as int64 (3,)."""
        out = torch.empty(3, dtype=torch.int64, device=self.device)
        L.check(self._lib.oth_counts_vs(self._h, _ptr(out), int(bool(reset)), self._stream()), "oth_counts_vs")
        return out

    # ------------------------------------------------------ Monte-Carlo playouts
    def playouts(self, n_playouts, per_move=False, seed=None, id_key=0, counter=None, score=False, best=False):
        """n_playouts random games to the end from every board's position
        (per_move=False: oth_playouts OTH_PLAYOUT_ROOT) or from the position after
        each of its possible moves (per_move=True: OTH_PLAYOUT_MOVES), on private
        copies: the boards, the ply counter and the tallies are left untouched.

        Returns wdl, then score and best when asked: int32 tensors on this device,
          wdl   (E, 3) or (E, N*N, 3): {wins, draws, losses} from the side to move
                at the root; zeros for squares that are not possible moves and for
                terminated boards;
          score (E,) or (E, N*N): the summed final disc difference (root mover's
                minus opponent's);
          best  (E,), per_move only: the possible move of the largest wins - losses
                (lowest square on ties), -1 without one.
        seed=None: the env's seed XOR PLAYOUT_SEED_XOR, so the draws never share a
        Philox key with the env's own play.  counter=None: `playout_counter`,
        which then moves on by one; the same (seed, id_key, counter) repeats the
        same playouts (include/othello_mi355x.h gives the draw of every ply)."""
        R = int(n_playouts)
        nn = self.board_size * self.board_size
        if best and not per_move:
            raise ValueError("best is the best possible move: it needs per_move=True")
        key = (self.seed ^ PLAYOUT_SEED_XOR if seed is None else int(seed)) & (2 ** 64 - 1)
        own = counter is None
        ctr = self._playout_calls if own else int(counter)
        shape = (self.num_envs, nn) if per_move else (self.num_envs,)
        wdl = self._i32(*(shape + (3,)))
        sc = self._i32(*shape) if score else None
        bt = self._i32(self.num_envs) if best else None
        L.check(self._lib.oth_playouts(self._h, L.OTH_PLAYOUT_MOVES if per_move else L.OTH_PLAYOUT_ROOT, R, key,
                                       int(id_key) & 0xffffffff, ctr, _ptr(wdl), _ptr(sc), _ptr(bt), self._stream()),
                "oth_playouts")
        if own:
            self._playout_calls += 1
        res = (wdl,) + ((sc,) if score else ()) + ((bt,) if best else ())
        return res[0] if len(res) == 1 else res

    def playout_actions(self, n_playouts, **kw):
        """Flat Monte-Carlo move selection: every board's possible move with the
        largest wins - losses over n_playouts random games each (playouts(per_move=True,
        best=True)); int32 (E,), -1 for a board without a possible move."""
        kw.pop("per_move", None)
        kw.pop("best", None)
        return self.playouts(n_playouts, per_move=True, best=True, **kw)[-1]

    @property
    def playout_counter(self):
        """`counter` of the next playouts() call that does not give one."""
        return self._playout_calls

    @playout_counter.setter
    def playout_counter(self, v):
        self._playout_calls = int(v)

    # ------------------------------------------------------ Monte-Carlo tree search
    def mcts(self, iterations, playouts=8, c=1.0, max_tree_nodes=None, seed=None, id_key=0, counter=None,
             wins2=False, best=False, tree_nodes=False, status=False):
        """A UCT-style tree search with random-playout leaf evaluation from every
        board's position (oth_mcts; include/othello_mi355x.h defines every output in
        integers): `iterations` descents, each evaluating one node with `playouts`
        (<= 64) random games, exploration constant c (round(256 c) in the key).  The
        boards, the ply counter and the tallies are left untouched.

        Returns visits, then wins2, best, tree_nodes and status when asked (the
        header's order), as tensors on this device:
          visits     int32 (E, N*N): the iterations through the root's child on each
                     square, 0 without a child -- the visit-count policy target;
          wins2      int32 (E, N*N): 2 wins + draws of the playouts backed up through
                     it, for the side to move at the root;
          best       int32 (E,): the most visited child (then the larger wins2, then
                     the lowest square), -1 without a possible move;
          tree_nodes int32 (E,): node slots the board's tree used;
          status     uint8 (E,): OTH_MCTS_DONE / TERMINATED / NO_MOVE.
        max_tree_nodes (per board) bounds the tree: a node whose children do not fit
        stays a leaf.  None: max(N*N, iterations (N*N - 4) / 4), clipped to the C
        ABI's maximum -- an iteration reserves at most one node's children.  This
        default started as a guess; tools/probe_mcts.py then found 8,185 8x8 mid-game
        boards at 64 iterations using 57 to 320 of its 960 slots, and one board at
        4,096 iterations 13,147 of 61,440, so it is 3 to 7
        times what those boards need; other board sizes are unmeasured.  The workspace
        (oth_mcts_workspace_bytes) is a cached uint8 tensor, regrown only when too
        small, so a warm call allocates nothing but its outputs and is capturable.
        seed=None / counter=None: as playouts() -- the env's seed XOR
        PLAYOUT_SEED_XOR, and `playout_counter`, which then moves on by one."""
        E, nn = self.num_envs, self.board_size * self.board_size
        I = int(iterations)
        if max_tree_nodes is None:
            max_tree_nodes = min(max(nn, I * (nn - 4) // 4), L.OTH_MCTS_MAX_TREE_NODES)
        key = (self.seed ^ PLAYOUT_SEED_XOR if seed is None else int(seed)) & (2 ** 64 - 1)
        own = counter is None
        ctr = self._playout_calls if own else int(counter)
        cx = int(round(256 * float(c)))
        for name, v in (("iterations", I), ("playouts", int(playouts)), ("c", cx),
                        ("max_tree_nodes", int(max_tree_nodes))):
            if not -2 ** 31 <= v < 2 ** 31:
                raise ValueError("%s is out of range" % name)
        if not 0 <= ctr < 2 ** 64:
            raise ValueError("counter is out of range")
        p = L.OthMctsParams(I, int(playouts), cx, int(max_tree_nodes), key, int(id_key) & 0xffffffff, ctr)
        need = ctypes.c_uint64(0)
        L.check(self._lib.oth_mcts_workspace_bytes(self.board_size, E, p.max_tree_nodes, ctypes.byref(need)),
                "oth_mcts_workspace_bytes")
        if self._mcts_ws is None or self._mcts_ws.numel() < need.value:
            self._mcts_ws = None  # (the old one goes first)
            self._mcts_ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        vis = self._i32(E, nn)
        w2 = self._i32(E, nn) if wins2 else None
        bt = self._i32(E) if best else None
        tn = self._i32(E) if tree_nodes else None
        stt = self._u8(E) if status else None
        L.check(self._lib.oth_mcts(self._h, ctypes.byref(p), _ptr(self._mcts_ws), self._mcts_ws.numel(), _ptr(vis),
                                   _ptr(w2), _ptr(bt), _ptr(tn), _ptr(stt), self._stream()), "oth_mcts")
        if own:
            self._playout_calls += 1
        res = (vis,) + tuple(t for t in (w2, bt, tn, stt) if t is not None)
        return res[0] if len(res) == 1 else res

    def mcts_actions(self, iterations, **kw):
        """Every board's most visited root move of mcts(iterations, **kw) (its `best`):
        int32 (E,), -1 for a board without a possible move."""
        for k in ("wins2", "best", "tree_nodes", "status"):
            kw.pop(k, None)
        return self.mcts(iterations, best=True, **kw)[1]

    # ------------------------------------------------ network-guided tree search
    def puct_begin(self, c=1.25, max_tree_nodes=None, layout="make_state", dtype=torch.float32):
        """Begin a network-guided tree search from every board's position
        (oth_puct_begin; include/othello_mi355x.h defines every step in integers):
        exploration constant c (round(256 c) in the key), max_tree_nodes node slots
        per board (None: max(N*N, 64 (N*N - 4)), what 256 simulations can reserve at
        most).  Returns the leaves to evaluate, a PuctLeaves of tensors on this device:
          kind   uint8 (E,): OTH_PUCT_LEAF_EXPAND (priors and value wanted), VALUE
                 (value only), TERMINAL (nothing), NONE (the board has no pending leaf);
          boards int64 (E, 2W), meta int16 (E,), legal int64 (E, W): the leaves in
                 the exchange format of get_state / set_state (a board without a
                 pending leaf shows its root, so every row is a valid input);
          obs    observe(layout, dtype) of those positions (layout=None: none).
        These tensors belong to the search: every puct_advance writes the next
        leaves into them in place (so a captured advance keeps feeding the same
        network input), and the next puct_begin makes new ones.  The boards, the
        ply counter and the tallies are left untouched.  The tree lives in a cached
        workspace of its own (not mcts()'s, whose call would overwrite a search in
        progress), regrown only when too small."""
        p, lv, leaves = self._puct_setup(1, c, max_tree_nodes, layout, dtype)
        L.check(self._lib.oth_puct_begin(self._h, ctypes.byref(p), _ptr(self._puct_ws), self._puct_ws.numel(),
                                         ctypes.byref(lv), self._stream()), "oth_puct_begin")
        self._puct, self._puct_k = (p, lv, leaves), 0
        return leaves

    def _puct_setup(self, K, c, max_tree_nodes, layout, dtype, batch=False):
        """What puct_begin and puct_begin_batch share: the parameters, the workspace (regrown only when
        too small) and new leaf tensors of E K rows.  The search in progress is dropped."""
        E, nn = self.num_envs, self.board_size * self.board_size
        K = int(K)
        if not 1 <= K <= L.OTH_PUCT_MAX_LEAVES:
            raise ValueError("leaves_per_board must be in [1, %d]" % L.OTH_PUCT_MAX_LEAVES)
        R = E * K
        if max_tree_nodes is None:
            max_tree_nodes = min(max(nn, 64 * (nn - 4)), L.OTH_PUCT_MAX_TREE_NODES)
        cx = int(round(256 * float(c)))
        for name, v in (("c", cx), ("max_tree_nodes", int(max_tree_nodes))):
            if not -2 ** 31 <= v < 2 ** 31:
                raise ValueError("%s is out of range" % name)
        p = L.OthPuctParams(cx, int(max_tree_nodes))
        obs = None
        lay = 0
        if layout is not None:
            lay = _OBS_LAYOUTS.get(layout, -1) if isinstance(layout, str) else int(layout)
            if lay not in _OBS_PLANES or dtype not in _DTYPES:
                raise ValueError("unknown observation layout %r or dtype %r" % (layout, dtype))
            obs = torch.empty((R,) + tuple(self._obs_shape(lay)[1:]), dtype=dtype, device=self.device)
        need = ctypes.c_uint64(0)
        if not batch:
            L.check(self._lib.oth_puct_workspace_bytes(self.board_size, E, p.max_tree_nodes, ctypes.byref(need)),
                    "oth_puct_workspace_bytes")
        else:
            L.check(self._lib.oth_puct_batch_workspace_bytes(self.board_size, E, p.max_tree_nodes, K,
                                                             ctypes.byref(need)), "oth_puct_batch_workspace_bytes")
        if self._puct_ws is None or self._puct_ws.numel() < need.value:
            self._puct_ws = None  # (the old one goes first)
            self._puct_ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        leaves = PuctLeaves(self._u8(R), torch.empty(R, 2 * self.words, dtype=torch.int64, device=self.device),
                            torch.empty(R, dtype=torch.int16, device=self.device),
                            torch.empty(R, self.words, dtype=torch.int64, device=self.device), obs)
        lv = L.OthPuctLeaves(leaves.kind.data_ptr(), leaves.boards.data_ptr(), leaves.meta.data_ptr(),
                             leaves.legal.data_ptr(), None if obs is None else obs.data_ptr(), lay,
                             _DTYPES[dtype] if obs is not None else 0)
        self._puct = None
        return p, lv, leaves

    def _puct_state(self, batch=None):
        """The search in progress; batch False / True: it must be one of the plain / the batch calls."""
        if self._puct is None:
            raise RuntimeError("no search in progress: call puct_begin() first")
        if batch is not None and batch != (self._puct_k > 0):
            raise RuntimeError("a search goes on with the calls that began it: this one was begun by %s"
                               % ("puct_begin_batch()" if self._puct_k > 0 else "puct_begin()"))
        return self._puct

    def puct_advance(self, priors, values, more=True):
        """One simulation of every board's search (oth_puct_advance): the pending
        leaves take their evaluation -- priors int32 (E, N*N) in [0, 65535] (read at
        the leaf's legal squares only; 65535 is probability 1), values int32 (E,) in
        [-32768, 32768] for the leaf's side to move, both as puct_quantize makes
        them -- are expanded and backed up, and, unless more is false, each search
        descends to its next leaf.  Returns puct_begin's PuctLeaves, rewritten in
        place.  int32 tensors on this device are passed as they are (a captured
        advance reads them again at every replay); others are converted first."""
        p, lv, leaves = self._puct_state(False)
        E, nn = self.num_envs, self.board_size * self.board_size
        pr = priors.to(device=self.device, dtype=torch.int32).contiguous()
        vl = values.to(device=self.device, dtype=torch.int32).contiguous()
        if pr.numel() != E * nn or vl.numel() != E:
            raise ValueError("priors must have %d elements and values %d" % (E * nn, E))
        L.check(self._lib.oth_puct_advance(self._h, ctypes.byref(p), _ptr(self._puct_ws), self._puct_ws.numel(),
                                           _ptr(pr), _ptr(vl), int(bool(more)), ctypes.byref(lv), self._stream()),
                "oth_puct_advance")
        return leaves

    def puct_result(self, value_sums=False, best=False, tree_nodes=False, status=False):
        """The search's outputs so far (oth_puct_result; it may be called at any point
        and changes nothing): visits, then value_sums, best, tree_nodes and status when
        asked (the header's order), as tensors on this device:
          visits     int32 (E, N*N): the simulations through the root's child on each
                     square, 0 without a child -- the visit-count policy target;
          value_sums int64 (E, N*N): the sum of the values backed up through it, in
                     units of 2^-15, for the side to move at the root;
          best       int32 (E,): the most visited child (then the larger value sum,
                     then the lowest square), -1 while no child has a visit;
          tree_nodes int32 (E,): node slots the board's tree used;
          status     uint8 (E,): OTH_MCTS_DONE / TERMINATED / NO_MOVE."""
        p, lv, leaves = self._puct_state()
        E, nn = self.num_envs, self.board_size * self.board_size
        vis = self._i32(E, nn)
        vs = torch.empty(E, nn, dtype=torch.int64, device=self.device) if value_sums else None
        bt = self._i32(E) if best else None
        tn = self._i32(E) if tree_nodes else None
        stt = self._u8(E) if status else None
        L.check(self._lib.oth_puct_result(self._h, ctypes.byref(p), _ptr(self._puct_ws), self._puct_ws.numel(),
                                          _ptr(vis), _ptr(vs), _ptr(bt), _ptr(tn), _ptr(stt), self._stream()),
                "oth_puct_result")
        res = (vis,) + tuple(t for t in (vs, bt, tn, stt) if t is not None)
        return res[0] if len(res) == 1 else res

    def puct_search(self, evaluate, simulations, **kw):
        """The whole loop: puct_begin, then `simulations` times evaluate(leaves) ->
        (logits (E, N*N), values (E,)) -- any callable, a torch module's forward on
        leaves.obs for example -- quantised by puct_quantize and given to
        puct_advance (more=False on the last), then puct_result.  c,
        max_tree_nodes (None: what `simulations` can reserve at most), layout and
        dtype go to puct_begin, value_sums / best / tree_nodes / status to
        puct_result, whose outputs are returned.  evaluate's floats are the only ones
        anywhere: given the integers puct_quantize makes of them, the search is exact.
        An evaluator whose `quantized` attribute is true (net.DeviceNet) returns the
        advance's (priors, values) itself and puct_quantize is not called: then there
        is no float at all, and layout=None saves the observation.

        leaves_per_board=K > 1: the batch calls (puct_begin_batch, puct_advance_batch with
        sim_limit = simulations), launched until no slot holds a leaf, so evaluate sees E K
        rows a call and is called about simulations / K times; every searched board ends
        with exactly `simulations` simulations.  Whether a leaf is left is one small
        read-back per launch: this path synchronises and refuses a HIP-graph capture.

        noise=RootNoise(...) (a keyword, default None): Dirichlet root noise, drawn on the
        device in integers -- the priors of the first advance go through puct_noise in
        leaf mode, which reaches exactly the boards whose pending leaf is the root.
        Without the keyword not one launch is added."""
        S = int(simulations)
        if S < 1:
            raise ValueError("simulations must be >= 1")
        K = int(kw.pop("leaves_per_board", 1))
        noise = kw.pop("noise", None)
        begin = dict((k, kw.pop(k)) for k in ("c", "max_tree_nodes", "layout", "dtype") if k in kw)
        if begin.get("max_tree_nodes") is None:
            nn = self.board_size * self.board_size
            begin["max_tree_nodes"] = min(max(nn, S * (nn - 4) // 4 + nn), L.OTH_PUCT_MAX_TREE_NODES)
        if K != 1:
            _no_capture("puct_search(leaves_per_board > 1)")
            leaves = self.puct_begin_batch(K, **begin)
            self._puct_run_batch(evaluate, leaves, S, noise)
            return self.puct_result(**kw)
        leaves = self.puct_begin(**begin)
        for i in range(S):
            priors, vals = _puct_evaluate(evaluate, leaves)
            if i == 0 and noise is not None:
                priors = self._puct_leaf_noise(noise, priors, leaves, 1)
            leaves = self.puct_advance(priors, vals, more=i < S - 1)
        return self.puct_result(**kw)

    def puct_actions(self, evaluate, simulations, **kw):
        """Every board's most visited root move of puct_search(evaluate, simulations,
        **kw) (its `best`): int32 (E,), -1 for a board without a possible move (or
        with simulations = 1, which evaluates the root alone)."""
        for k in ("value_sums", "best", "tree_nodes", "status"):
            kw.pop(k, None)
        return self.puct_search(evaluate, simulations, best=True, **kw)[1]

    # ---------------------------------------------- K leaves a board per launch
    def puct_begin_batch(self, leaves_per_board, c=1.25, max_tree_nodes=None, layout="make_state",
                         dtype=torch.float32):
        """puct_begin for a search that emits up to K = leaves_per_board leaves a board per launch
        under virtual loss (oth_puct_begin_batch; the header defines the merge in integers, one
        board's slots in ascending order).  The PuctLeaves it returns has E K rows, row e K + j slot
        j of board e, so any evaluator works unchanged on a batch of E K; a slot without a leaf has
        kind NONE and shows the root.  Here the root is slot 0's leaf.  The search goes on with
        puct_advance_batch and puct_reroot_batch; puct_result and puct_pick serve both families."""
        K = int(leaves_per_board)
        p, lv, leaves = self._puct_setup(K, c, max_tree_nodes, layout, dtype, batch=True)
        L.check(self._lib.oth_puct_begin_batch(self._h, ctypes.byref(p), K, _ptr(self._puct_ws),
                                               self._puct_ws.numel(), ctypes.byref(lv), self._stream()),
                "oth_puct_begin_batch")
        self._puct, self._puct_k = (p, lv, leaves), K
        return leaves

    def puct_advance_batch(self, priors, values, sim_limit=None):
        """One launch of a batch search (oth_puct_advance_batch): every slot's leaf takes its row of
        priors int32 (E K, N*N) and values int32 (E K,), in slot order; then each board selects up
        to K new leaves under virtual loss, none beyond sim_limit simulations at its root in all
        (None: no limit; 0: none at all, puct_advance's more=False).  A board's batch closes early
        where a selection meets a leaf already taken in this launch.  Returns the PuctLeaves,
        rewritten in place."""
        p, lv, leaves = self._puct_state(True)
        K = self._puct_k
        R, nn = self.num_envs * K, self.board_size * self.board_size
        pr = priors.to(device=self.device, dtype=torch.int32).contiguous()
        vl = values.to(device=self.device, dtype=torch.int32).contiguous()
        if pr.numel() != R * nn or vl.numel() != R:
            raise ValueError("priors must have %d elements and values %d" % (R * nn, R))
        lim = L.OTH_PUCT_MAX_SIMS if sim_limit is None else int(sim_limit)
        if not 0 <= lim <= L.OTH_PUCT_MAX_SIMS:
            raise ValueError("sim_limit is out of range")
        L.check(self._lib.oth_puct_advance_batch(self._h, ctypes.byref(p), K, _ptr(self._puct_ws),
                                                 self._puct_ws.numel(), _ptr(pr), _ptr(vl), lim, ctypes.byref(lv),
                                                 self._stream()), "oth_puct_advance_batch")
        return leaves

    def puct_reroot_batch(self, actions, root_priors=None, kept=False, sim_limit=None):
        """puct_reroot for a batch search (oth_puct_reroot_batch): every slot's leaf is dropped, and
        each searched board selects up to K leaves from its new root, within sim_limit (a kept
        root's visits count).  A fresh or unexpanded root is slot 0's leaf alone."""
        p, lv, leaves = self._puct_state(True)
        K = self._puct_k
        E, nn = self.num_envs, self.board_size * self.board_size
        a = actions.to(device=self.device, dtype=torch.int32).contiguous()
        if a.numel() != E:
            raise ValueError("expected %d actions, got %d" % (E, a.numel()))
        rp = None
        if root_priors is not None:
            rp = root_priors.to(device=self.device, dtype=torch.int32).contiguous()
            if rp.numel() != E * nn:
                raise ValueError("root_priors must have %d elements" % (E * nn))
        lim = L.OTH_PUCT_MAX_SIMS if sim_limit is None else int(sim_limit)
        if not 0 <= lim <= L.OTH_PUCT_MAX_SIMS:
            raise ValueError("sim_limit is out of range")
        kp = self._u8(E) if kept else None
        L.check(self._lib.oth_puct_reroot_batch(self._h, ctypes.byref(p), K, _ptr(self._puct_ws),
                                                self._puct_ws.numel(), _ptr(a), _ptr(rp), _ptr(kp), lim,
                                                ctypes.byref(lv), self._stream()), "oth_puct_reroot_batch")
        return (leaves, kp) if kept else leaves

    def _puct_run_batch(self, evaluate, leaves, S, noise=None):
        """Launches with sim_limit = S until no slot holds a leaf (one read-back of kind.any() a launch).
        noise: root noise on the first launch's priors, where a slot 0 holds the root."""
        first = True
        while bool(leaves.kind.any()):
            priors, vals = _puct_evaluate(evaluate, leaves)
            if first and noise is not None:
                priors = self._puct_leaf_noise(noise, priors, leaves, self._puct_k)
            first = False
            leaves = self.puct_advance_batch(priors, vals, sim_limit=S)
        return leaves

    # ------------------------------------------------- self-play on the search's tree
    def puct_pick(self, sample=None, seed=None, counter=None):
        """The move of the search so far for every board (oth_puct_pick; it changes
        nothing and may be called at any point): int32 (E,).  sample None or 0 for a
        board: puct_result's `best`; sample (a bool / uint8 (E,) tensor, or True for
        every board) nonzero: a square drawn in proportion to the root's children's
        visits -- temperature 1, the self-play move of the opening plies -- by a
        stateless Philox draw keyed by (seed, global env id, counter), so a sharded
        run equals the unsharded one.  -1 for a board that is terminated, has no
        possible move, or whose root has no visited child yet.  seed=None: the env's
        seed XOR PLAYOUT_SEED_XOR; counter=None: `puct_pick_counter`, which then
        moves on by one (only when a sample is asked for)."""
        p, lv, leaves = self._puct_state()
        E = self.num_envs
        sm = None
        if sample is True:
            sm = torch.ones(E, dtype=torch.uint8, device=self.device)
        elif sample is not None and sample is not False:
            sm = sample.to(device=self.device).ne(0).to(torch.uint8).contiguous()
            if sm.numel() != E:
                raise ValueError("sample must have %d elements" % E)
        key = (self.seed ^ PLAYOUT_SEED_XOR if seed is None else int(seed)) & (2 ** 64 - 1)
        own = counter is None
        ctr = self._pick_calls if own else int(counter)
        if not 0 <= ctr < 2 ** 64:
            raise ValueError("counter is out of range")
        actions = self._i32(E)
        L.check(self._lib.oth_puct_pick(self._h, ctypes.byref(p), _ptr(self._puct_ws), self._puct_ws.numel(), _ptr(sm),
                                        key, 0, ctr, _ptr(actions), self._stream()), "oth_puct_pick")
        if own and sm is not None:
            self._pick_calls += 1
        return actions

    @property
    def puct_pick_counter(self):
        """`counter` of the next sampling puct_pick() call that does not give one."""
        return self._pick_calls

    @puct_pick_counter.setter
    def puct_pick_counter(self, v):
        self._pick_calls = int(v)

    # ------------------------------------------------------------- root noise
    def puct_noise(self, priors, epsilon, table, leaves=None, rows_per_board=1, out=None, seed=None, id_key=0,
                   counter=None):
        """Dirichlet root noise mixed into rows of priors, in integers (oth_puct_noise;
        the header defines the draw and the mix).  priors int32 (E K, N*N), K =
        rows_per_board; epsilon an int in [0, 256], in units of 1/256; table int32
        (4096,), noise.dirichlet_table's.  Row e K of board e becomes ((256 - epsilon)
        clamp(p, 0, 65535) + epsilon eta + 128) >> 8 on the squares of the handle's
        possible_moves, eta the normalised table draws of those squares; every other
        row and square is copied.

        leaves None ("root mode"): every board takes noise -- for the root_priors of
        puct_reroot, from an evaluation of the handle's position.  leaves a PuctLeaves
        ("leaf mode"): only where the leaf of row e K is an EXPAND leaf on the handle's
        own board, that is, where the pending leaf is the root -- for the priors of the
        first advance of a move.

        out None: a new tensor; out a contiguous int32 tensor on this device of the
        same size (it may be `priors` itself: in place).  The draws are keyed by (seed,
        global env id + id_key, counter, square): a sharded run equals the unsharded
        one.  seed=None: the env's seed XOR PLAYOUT_SEED_XOR; counter=None:
        `puct_noise_counter`, which then moves on by one.  The call reads the handle
        and a search's leaves, writes neither, and is capturable with the counter
        baked in."""
        E, nn = self.num_envs, self.board_size * self.board_size
        K = int(rows_per_board)
        if not 1 <= K <= L.OTH_PUCT_MAX_LEAVES:
            raise ValueError("rows_per_board must be in [1, %d]" % L.OTH_PUCT_MAX_LEAVES)
        eps = int(epsilon)
        if not 0 <= eps <= 256:
            raise ValueError("epsilon must be an integer in [0, 256] (units of 1/256)")
        pr = priors.to(device=self.device, dtype=torch.int32).contiguous()
        if pr.numel() != E * K * nn:
            raise ValueError("priors must have %d elements" % (E * K * nn))
        tb = table.to(device=self.device, dtype=torch.int32).contiguous()
        if tb.numel() != L.OTH_NOISE_TABLE:
            raise ValueError("table must have %d entries" % L.OTH_NOISE_TABLE)
        if out is None:
            out = torch.empty_like(pr)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.device != self.device or \
                not out.is_contiguous() or out.numel() != pr.numel():
            raise ValueError("out must be a contiguous int32 tensor of %d elements on %s" % (pr.numel(), self.device))
        kind = boards = None
        if leaves is not None:
            kind, boards = leaves.kind, leaves.boards
            if kind.dtype != torch.uint8 or boards.dtype != torch.int64 or kind.device != self.device or \
                    boards.device != self.device or not kind.is_contiguous() or not boards.is_contiguous() or \
                    kind.numel() != E * K or boards.numel() != E * K * 2 * self.words:
                raise ValueError("leaves must be a PuctLeaves of %d rows on %s" % (E * K, self.device))
        key = (self.seed ^ PLAYOUT_SEED_XOR if seed is None else int(seed)) & (2 ** 64 - 1)
        own = counter is None
        ctr = self._noise_calls if own else int(counter)
        if not 0 <= ctr < 2 ** 64:
            raise ValueError("counter is out of range")
        L.check(self._lib.oth_puct_noise(self._h, K, _ptr(kind), _ptr(boards), _ptr(pr), _ptr(out), eps, _ptr(tb), key,
                                         int(id_key) & 0xffffffff, ctr, self._stream()), "oth_puct_noise")
        if own:
            self._noise_calls += 1
        return out

    @property
    def puct_noise_counter(self):
        """`counter` of the next puct_noise() call that does not give one."""
        return self._noise_calls

    @puct_noise_counter.setter
    def puct_noise_counter(self, v):
        self._noise_calls = int(v)

    def _puct_leaf_noise(self, noise, priors, leaves, K):
        """A move's first advance under `noise` (a noise.RootNoise): the leaf-mode call on the evaluator's
        priors, in place where they are the int32 rows the advance takes."""
        own = priors.dtype == torch.int32 and priors.device == self.device and priors.is_contiguous()
        return self.puct_noise(priors, noise.epsilon, noise.table_on(self.device), leaves=leaves, rows_per_board=K,
                               out=priors if own else None)

    def _puct_root_noise(self, noise, evaluate):
        """puct_play's root_priors under `noise`: one more evaluation, of the stepped handle's position (its
        get_state rows as a PuctLeaves, with the observation of the search's layout where it has one), through
        the root-mode call."""
        _, lv, leaves = self._puct_state()
        boards, meta, legal = self.get_state()
        obs = None if leaves.obs is None else self.observe(int(lv.layout), leaves.obs.dtype)
        kind = torch.full((self.num_envs,), L.OTH_PUCT_LEAF_EXPAND, dtype=torch.uint8, device=self.device)
        priors, _ = _puct_evaluate(evaluate, PuctLeaves(kind, boards, meta, legal, obs))
        own = priors.dtype == torch.int32 and priors.device == self.device and priors.is_contiguous()
        return self.puct_noise(priors, noise.epsilon, noise.table_on(self.device), out=priors if own else None)

    def puct_reroot(self, actions, root_priors=None, kept=False):
        """Carry the search to the position the handle has reached since it began --
        normally by step(actions) -- keeping the subtree of the played move
        (oth_puct_reroot).  actions int32 (E,): the squares that were played.  A
        board is kept if the root's child on actions[e] is the handle's position
        (discs, side to move, possible moves) and the game goes on; then that child
        is the new root, with every node below it as it was, and the rest of the
        tree's slots are free again.  Any other board -- a game that ended or
        auto-reset, an action of -1, a handle set elsewhere -- begins afresh from
        the handle's position, exactly as puct_begin would.  root_priors int32 (E,
        N*N) (as puct_quantize makes them): the new priors of the kept roots'
        children, the way to mix root noise in again; fresh roots take theirs at
        their first advance.  Returns the search's PuctLeaves, rewritten in place
        with every board's next leaf; with kept=True (the leaves, kept uint8 (E,))."""
        p, lv, leaves = self._puct_state(False)
        E, nn = self.num_envs, self.board_size * self.board_size
        a = actions.to(device=self.device, dtype=torch.int32).contiguous()
        if a.numel() != E:
            raise ValueError("expected %d actions, got %d" % (E, a.numel()))
        rp = None
        if root_priors is not None:
            rp = root_priors.to(device=self.device, dtype=torch.int32).contiguous()
            if rp.numel() != E * nn:
                raise ValueError("root_priors must have %d elements" % (E * nn))
        kp = self._u8(E) if kept else None
        L.check(self._lib.oth_puct_reroot(self._h, ctypes.byref(p), _ptr(self._puct_ws), self._puct_ws.numel(), _ptr(a),
                                          _ptr(rp), _ptr(kp), ctypes.byref(lv), self._stream()), "oth_puct_reroot")
        return (leaves, kp) if kept else leaves

    def puct_play(self, evaluate, simulations, sample=None, **begin_kw):
        """One move of self-play on every board: puct_begin(**begin_kw) if no search is
        in progress, `simulations` advances with evaluate(leaves) -> (logits, values)
        as puct_search runs them (the last with more=False), puct_result's visits,
        puct_pick(sample), step(actions, observe=False) and puct_reroot(actions), so
        that the next call goes on from the played child's subtree.  Returns
        PuctPlay(actions, visits, rewards, dones, kept): visits int32 (E, N*N) is the
        policy target of the position the move was played from.

        A board whose action is -1 (terminated, without a possible move, or
        simulations = 1) steps as any action outside possible_moves does: a
        terminated board is left as it is and reports done (with auto_reset it was
        reset at its terminal ply and never shows up terminated); a live board takes
        the invalid-move path -- the mover loses at once under
        sudden_death_on_invalid_move, otherwise the turn passes.  Its search begins
        afresh.  max_tree_nodes=None: twice what `simulations` can reserve, since a
        kept subtree comes on top of a move's own expansions; a full tree only stops
        growing (VALUE leaves).

        leaves_per_board=K > 1 (among begin_kw): the batch calls, as puct_search runs them,
        with sim_limit = simulations in every launch and in the re-root; the visits a kept
        root brings along count, so a move adds what is missing to `simulations`.  This path
        reads kind.any() back once a launch and refuses a HIP-graph capture.

        record=True (a keyword beside begin_kw, default False): the move goes into the
        replay store (replay_begin first): replay_append(visits) before the step,
        replay_label(rewards, dones) after it.

        noise=RootNoise(...) (a keyword beside begin_kw, default None): Dirichlet root
        noise on every move's root, in integers on the device.  The priors of the
        call's first advance go through puct_noise in leaf mode (fresh roots and kept
        roots that are not expanded yet; other leaves are untouched); after the step
        the evaluator runs once more, on the stepped handle's position (get_state's
        rows as a PuctLeaves, with the observation of the search's layout where it has
        one), its priors go through puct_noise in root mode and are the re-root's
        root_priors, so a kept root's children take noise too.  puct_noise_counter moves
        on by one a call.  Without the keyword not one launch is added."""
        S = int(simulations)
        record = bool(begin_kw.pop("record", False))
        noise = begin_kw.pop("noise", None)
        if S < 1:
            raise ValueError("simulations must be >= 1")
        K = int(begin_kw.pop("leaves_per_board", 1))
        if self._puct is not None and max(self._puct_k, 1) != K:
            raise RuntimeError("the search in progress was begun with leaves_per_board=%d" % max(self._puct_k, 1))
        if self._puct is None:
            if begin_kw.get("max_tree_nodes") is None:
                nn = self.board_size * self.board_size
                begin_kw["max_tree_nodes"] = min(max(nn, 2 * (S * (nn - 4) // 4 + nn)), L.OTH_PUCT_MAX_TREE_NODES)
            if K != 1:
                self.puct_begin_batch(K, **begin_kw)
            else:
                self.puct_begin(**begin_kw)
        leaves = self._puct[2]
        if K != 1:
            _no_capture("puct_play(leaves_per_board > 1)")
            self._puct_run_batch(evaluate, leaves, S, noise)
            visits = self.puct_result()
            actions = self.puct_pick(sample)
            if record:
                self.replay_append(visits)
            _, rewards, dones, _ = self.step(actions, observe=False)
            if record:
                self.replay_label(rewards, dones)
            rp = None if noise is None else self._puct_root_noise(noise, evaluate)
            _, kept = self.puct_reroot_batch(actions, root_priors=rp, kept=True, sim_limit=S)
            return PuctPlay(actions, visits, rewards, dones, kept)
        for i in range(S):
            priors, vals = _puct_evaluate(evaluate, leaves)
            if i == 0 and noise is not None:
                priors = self._puct_leaf_noise(noise, priors, leaves, 1)
            leaves = self.puct_advance(priors, vals, more=i < S - 1)
        visits = self.puct_result()
        actions = self.puct_pick(sample)
        if record:
            self.replay_append(visits)
        _, rewards, dones, _ = self.step(actions, observe=False)
        if record:
            self.replay_label(rewards, dones)
        rp = None if noise is None else self._puct_root_noise(noise, evaluate)
        _, kept = self.puct_reroot(actions, root_priors=rp, kept=True)
        return PuctPlay(actions, visits, rewards, dones, kept)

    # ------------------------------------------------------------ the replay store
    def replay_begin(self, horizon, max_batch=4096):
        """Begin an empty replay store for this env's boards (oth_replay_begin;
        include/othello_mi355x.h defines every call in integers): a ring of `horizon`
        record slots per board, row e * horizon + j being slot j of board e, and
        batches of at most `max_batch` rows.  The store lives in a cached workspace
        of its own, regrown only when too small."""
        H, B = int(horizon), int(max_batch)
        need = ctypes.c_uint64(0)
        L.check(self._lib.oth_replay_workspace_bytes(self.board_size, self.num_envs, H, B, ctypes.byref(need)),
                "oth_replay_workspace_bytes")
        if self._replay_ws is None or self._replay_ws.numel() < need.value:
            self._replay_ws = None  # (the old one goes first)
            self._replay_ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        L.check(self._lib.oth_replay_begin(self._h, H, B, _ptr(self._replay_ws), self._replay_ws.numel(),
                                           self._stream()), "oth_replay_begin")
        self._replay = (H, B)

    def _replay_args(self):
        if self._replay is None:
            raise RuntimeError("no replay store: call replay_begin() first")
        H, B = self._replay
        return self._h, H, B, _ptr(self._replay_ws), self._replay_ws.numel()

    def replay_append(self, visits, skip=None):
        """Record every live board's position with its visit target (oth_replay_append):
        visits int32 (E, N*N), cleaned to [0, 2^24 - 1] on the stored possible moves and
        0 elsewhere; a board records unless it is terminated, skip[e] (uint8 / bool (E,))
        is set or no cleaned visit is positive.  Call it before the step that plays the
        move.  int32 tensors on this device are passed as they are."""
        E, nn = self.num_envs, self.board_size * self.board_size
        v = visits.to(device=self.device, dtype=torch.int32).contiguous()
        if v.numel() != E * nn:
            raise ValueError("visits must have %d elements" % (E * nn))
        sk = None
        if skip is not None:
            sk = skip.to(device=self.device).ne(0).to(torch.uint8).contiguous()
            if sk.numel() != E:
                raise ValueError("skip must have %d elements" % E)
        L.check(self._lib.oth_replay_append(*self._replay_args(), _ptr(v), _ptr(sk), self._stream()),
                "oth_replay_append")

    def replay_label(self, rewards, dones):
        """Label the finished games (oth_replay_label): where dones[e] is set, every open
        record of board e's current game takes the outcome +rewards[e] (clamped to
        [-32768, 32768]) if its side to move is the side that moved at the latest
        append, else -rewards[e].  rewards and dones are what step() returned for the
        ply played from the latest appended position."""
        E = self.num_envs
        r = rewards.to(device=self.device, dtype=torch.int32).contiguous()
        d = dones.to(device=self.device)
        d = (d if d.dtype == torch.uint8 else d.ne(0).to(torch.uint8)).contiguous()
        if r.numel() != E or d.numel() != E:
            raise ValueError("rewards and dones must have %d elements" % E)
        L.check(self._lib.oth_replay_label(*self._replay_args(), _ptr(r), _ptr(d), self._stream()),
                "oth_replay_label")

    def replay_counts(self):
        """int64 (3,) on this device: the rows that are empty, open and labelled (oth_replay_counts)."""
        out = torch.empty(3, dtype=torch.int64, device=self.device)
        L.check(self._lib.oth_replay_counts(*self._replay_args(), _ptr(out), self._stream()), "oth_replay_counts")
        return out

    def _replay_batch(self, n, layout, dtype, fields):
        """New tensors of n rows for a batch, and its C struct.  fields None: all of them."""
        W, nn, dev = self.words, self.board_size * self.board_size, self.device
        want = ReplayBatch._fields if fields is None else tuple(fields)
        unknown = set(want) - set(ReplayBatch._fields)
        if unknown:
            raise ValueError("unknown batch fields %s" % sorted(unknown))
        obs, lay = None, 0
        if layout is not None and "obs" in want:
            lay = _OBS_LAYOUTS.get(layout, -1) if isinstance(layout, str) else int(layout)
            if lay not in _OBS_PLANES or dtype not in _DTYPES:
                raise ValueError("unknown observation layout %r or dtype %r" % (layout, dtype))
            obs = torch.empty((n,) + tuple(self._obs_shape(lay)[1:]), dtype=dtype, device=dev)
        shapes = dict(state=((n,), torch.uint8), boards=((n, 2 * W), torch.int64), meta=((n,), torch.int16),
                      legal=((n, W), torch.int64), visits=((n, nn), torch.int32), outcome=((n,), torch.int32),
                      rows=((n,), torch.int32), sym=((n,), torch.uint8))
        t = {k: torch.empty(sh, dtype=dt, device=dev) if k in want else None for k, (sh, dt) in shapes.items()}
        batch = ReplayBatch(t["state"], t["boards"], t["meta"], t["legal"], t["visits"], t["outcome"], obs, t["rows"],
                            t["sym"])
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        c = L.OthReplayBatch(ptr(batch.state), ptr(batch.boards), ptr(batch.meta), ptr(batch.legal), ptr(batch.visits),
                             ptr(batch.outcome), ptr(obs), lay, _DTYPES[dtype] if obs is not None else 0,
                             ptr(batch.rows), ptr(batch.sym))
        return batch, c

    def replay_gather(self, rows, sym=None, layout="make_state", dtype=torch.float32, fields=None):
        """The store's rows `rows` (int32 (n,), n <= max_batch) under the symmetries `sym`
        (uint8 (n,), the low three bits; None: the identity) as a ReplayBatch of tensors
        on this device (oth_replay_gather): state uint8 (n,), boards int64 (n, 2W), meta
        int16 (n,), legal int64 (n, W) in the exchange format, visits int32 (n, N*N),
        outcome int32 (n,) from the row's mover's side, obs = observe(layout, dtype) of
        those positions (layout=None: none), and rows / sym as used (-1: a row number
        outside the store, which gives an empty row: zeros).  fields: the names to make
        (the others are None and cost nothing)."""
        r = rows.to(device=self.device, dtype=torch.int32).contiguous()
        n = r.numel()
        sm = None
        if sym is not None:
            sm = sym.to(device=self.device, dtype=torch.uint8).contiguous()
            if sm.numel() != n:
                raise ValueError("sym must have %d elements" % n)
        batch, c = self._replay_batch(n, layout, dtype, fields)
        L.check(self._lib.oth_replay_gather(*self._replay_args(), n, _ptr(r), _ptr(sm), ctypes.byref(c),
                                            self._stream()), "oth_replay_gather")
        return batch

    def replay_sample(self, n, augment=True, seed=None, counter=None, id_key=0, layout="make_state",
                      dtype=torch.float32, fields=None):
        """A minibatch of n labelled rows drawn uniformly with replacement, each under a
        random symmetry of the board when augment is set (oth_replay_sample): a
        stateless Philox draw keyed by (seed, id_key + i, counter) that depends on this
        store alone.  seed=None: the env's seed XOR PLAYOUT_SEED_XOR; counter=None:
        `replay_sample_counter`, which then moves on by one.  A store without a
        labelled row gives empty rows (rows -1).  Returns replay_gather's ReplayBatch."""
        n = int(n)
        key = (self.seed ^ PLAYOUT_SEED_XOR if seed is None else int(seed)) & (2 ** 64 - 1)
        own = counter is None
        ctr = self._replay_calls if own else int(counter)
        if not 0 <= ctr < 2 ** 64:
            raise ValueError("counter is out of range")
        if n < 1:
            raise ValueError("n must be >= 1")
        batch, c = self._replay_batch(n, layout, dtype, fields)
        L.check(self._lib.oth_replay_sample(*self._replay_args(), n, int(bool(augment)), key,
                                            int(id_key) & 0xFFFFFFFF, ctr, ctypes.byref(c), self._stream()),
                "oth_replay_sample")
        if own:
            self._replay_calls += 1
        return batch

    @property
    def replay_sample_counter(self):
        """`counter` of the next replay_sample() call that does not give one."""
        return self._replay_calls

    @replay_sample_counter.setter
    def replay_sample_counter(self, v):
        self._replay_calls = int(v)

    # ------------------------------------------------------------ exact endgame
    def solve(self, max_empties=10, max_nodes=1 << 22, best=False, move_values=False, status=False, nodes=False):
        """Exact endgame values (oth_solve): for every live board with at most
        max_empties (<= 14) empty squares, the final disc difference under best
        play by both sides, from the side to move; the boards, the ply counter and
        the tallies are left untouched, and no random number is drawn.

        Returns value, then best, move_values, status and nodes when asked (the
        header's order), as tensors on this device:
          value       int32 (E,); OTH_SOLVE_NO_VALUE (-32768) where there is none;
          best        int32 (E,): the lowest possible move that attains value, -1 without;
          move_values int32 (E, N*N): the value of every stored possible move;
          status      uint8 (E,): OTH_SOLVE_EXACT / TERMINATED / SKIPPED (more than
                      max_empties empty squares: no search) / NO_MOVE / ABORTED;
          nodes       int64 (E,) (the C ABI's uint64): disc placements searched.
        max_nodes bounds the search of one root move (status ABORTED beyond it).
        Its default started as a guess; tools/probe_solve.py then found no board
        over it among 65,536 random-play 8x8 positions with 10 empty squares (the
        largest board searched 9.0e5 nodes over all its moves) nor among 1,024 with
        12, so it stayed.  Other board sizes are unmeasured."""
        E, nn = self.num_envs, self.board_size * self.board_size
        val = self._i32(E)
        bt = self._i32(E) if best else None
        mv = self._i32(E, nn) if move_values else None
        stt = self._u8(E) if status else None
        nd = torch.empty(E, dtype=torch.int64, device=self.device) if nodes else None
        L.check(self._lib.oth_solve(self._h, int(max_empties), int(max_nodes), _ptr(val), _ptr(bt), _ptr(mv),
                                    _ptr(stt), _ptr(nd), self._stream()), "oth_solve")
        res = (val,) + tuple(t for t in (bt, mv, stt, nd) if t is not None)
        return res[0] if len(res) == 1 else res

    def solve_actions(self, **kw):
        """Every board's exactly best move (solve(best=True)'s `best`): int32 (E,),
        -1 where the solver gives none (see solve's status)."""
        for k in ("best", "move_values", "status", "nodes"):
            kw.pop(k, None)
        return self.solve(best=True, **kw)[1]

    # ------------------------------------------------------- depth-limited search
    def _search_weights(self, weights):
        """weights as the device int8 (N*N,) tensor oth_search reads."""
        nn = self.board_size * self.board_size
        if weights is None:  # moved to the device once: a captured call copies nothing
            if getattr(self, "_default_w", None) is None:
                self._default_w = default_search_weights(self.board_size).reshape(nn).to(self.device)
            return self._default_w
        return _int8_weights(weights, self.board_size).reshape(nn).to(self.device).contiguous()

    def search(self, depth, weights=None, mobility=0, terminal=64, max_nodes=1 << 22, best=False, move_values=False,
               status=False, nodes=False):
        """Depth-limited alpha-beta (oth_search) of every live board, whatever its
        number of empty squares: `depth` (1..14) discs ahead, the frontier valued by
        weighted squares plus mobility,
            sum_a weights[a] ([a mine] - [a theirs]) + mobility (my moves - their moves),
        and a game end by terminal * (my discs - their discs), all from the side to
        move; a pass consumes no depth.  weights: an (N, N) or (N*N,) integer tensor
        or array that fits int8 (None: default_search_weights(N)); mobility in
        [-127, 127]; terminal in [1, 32767].  The boards, the ply counter and the
        tallies are left untouched, and no random number is drawn.

        Returns value, then best, move_values, status and nodes when asked, as
        solve() does: value int32 (E,) with OTH_SEARCH_NO_VALUE (-2^31) where there
        is none; status OTH_SEARCH_DONE / TERMINATED / NO_MOVE / ABORTED (more than
        max_nodes disc placements under one root move).  max_nodes' default
        started as a guess; tools/probe_search.py then found no board over it at
        depths 1-5 among 65,536 random-play 8x8 positions with 30 empty squares nor
        with 20 (the largest board searched 5.3e5 nodes over all its moves at depth
        5), so it stayed.  Deeper searches and other board
        sizes are unmeasured."""
        E, nn = self.num_envs, self.board_size * self.board_size
        w = self._search_weights(weights)
        val = self._i32(E)
        bt = self._i32(E) if best else None
        mv = self._i32(E, nn) if move_values else None
        stt = self._u8(E) if status else None
        nd = torch.empty(E, dtype=torch.int64, device=self.device) if nodes else None
        L.check(self._lib.oth_search(self._h, int(depth), _ptr(w), int(mobility), int(terminal), int(max_nodes),
                                     _ptr(val), _ptr(bt), _ptr(mv), _ptr(stt), _ptr(nd), self._stream()),
                "oth_search")
        res = (val,) + tuple(t for t in (bt, mv, stt, nd) if t is not None)
        return res[0] if len(res) == 1 else res

    def search_actions(self, **kw):
        """Every board's best move of the search (search(best=True)'s `best`): int32
        (E,), -1 where the search gives none (see search's status)."""
        for k in ("best", "move_values", "status", "nodes"):
            kw.pop(k, None)
        return self.search(best=True, **kw)[1]

    def search_ntuple(self, depth, net, terminal=64, max_nodes=1 << 22, best=False, move_values=False, status=False,
                      nodes=False):
        """search() with a learned evaluation (oth_search_ntuple): the frontier is
        valued by `net` (an ntuple.NTupleNet for this board size on this device), its
        value from the side to move there, in [-32768, 32768]; a game end by terminal
        * (my discs - their discs).  Everything else -- rules, outputs, statuses,
        nodes, determinism -- is search()'s.  The net's weights are read as they are
        when the launch runs."""
        net._check_env(self)
        E, nn = self.num_envs, self.board_size * self.board_size
        val = self._i32(E)
        bt = self._i32(E) if best else None
        mv = self._i32(E, nn) if move_values else None
        stt = self._u8(E) if status else None
        nd = torch.empty(E, dtype=torch.int64, device=self.device) if nodes else None
        L.check(self._lib.oth_search_ntuple(self._h, int(depth), ctypes.byref(net.params), _ptr(net.plan),
                                            net.plan_bytes, _ptr(net._weights()), net.weight_count, int(terminal),
                                            int(max_nodes), _ptr(val), _ptr(bt), _ptr(mv), _ptr(stt), _ptr(nd),
                                            self._stream()), "oth_search_ntuple")
        res = (val,) + tuple(t for t in (bt, mv, stt, nd) if t is not None)
        return res[0] if len(res) == 1 else res

    def search_ntuple_actions(self, **kw):
        """Every board's best move of search_ntuple (its `best`): int32 (E,), -1 where
        the search gives none."""
        for k in ("best", "move_values", "status", "nodes"):
            kw.pop(k, None)
        return self.search_ntuple(best=True, **kw)[1]

    def _sampler_inputs(self, logits, uniforms):
        """(logits rows, uniforms) checked before a launch reads them: the rows on
        this handle's device, one per board; uniforms float32 on it, >= E of them."""
        x = _rows(logits, self.board_size)
        if x.device != self.device:
            raise ValueError("logits must be on %s (got %s)" % (self.device, x.device))
        if x.shape[0] != self.num_envs:
            raise ValueError("logits must have one row per board")
        if uniforms is not None:
            if uniforms.dtype != torch.float32 or not uniforms.is_contiguous() or uniforms.device != self.device:
                uniforms = uniforms.to(device=self.device, dtype=torch.float32).contiguous()
            if uniforms.numel() < self.num_envs:
                raise ValueError("uniforms must hold one value per board (%d), got %d" %
                                 (self.num_envs, uniforms.numel()))
        return x, uniforms

    def sample_actions(self, logits, deterministic=False, uniforms=None, log_probs=True, entropy=True):
        """Policy.act (model.py:60-99) for every board at once: sample (or, when
        deterministic, take the mode of) the softmax of `logits` (E, N*N)
        float32 restricted to the board's possible_moves.  Draws are Philox
        keyed (seed, env id, call counter) unless `uniforms` (E,) is given.
        Returns (actions int32, log_probs, entropy) on the device; the actions
        feed step() directly."""
        x, uniforms = self._sampler_inputs(logits, uniforms)
        acts = self._i32(self.num_envs)
        lp = torch.empty(self.num_envs, dtype=torch.float32, device=self.device) if log_probs else None
        ent = torch.empty(self.num_envs, dtype=torch.float32, device=self.device) if entropy else None
        mode = L.OTH_MASKED_MODE if deterministic else L.OTH_MASKED_SAMPLE
        L.check(self._lib.oth_sample_actions(self._h, _ptr(x), x.stride(0), _ptr(uniforms), self._sample_calls,
                                             mode, _ptr(acts), _ptr(lp), _ptr(ent), self._stream()),
                "oth_sample_actions")
        self._sample_calls += 1
        return acts, lp, ent

    def sample_step(self, logits, deterministic=False, uniforms=None, log_probs=True, entropy=True,
                    full_entropy=False, rewards=None, dones=None, actions=None, observe=None, obs=None,
                    obs_dtype=torch.float32):
        """sample_actions(logits) then step(actions) in ONE launch (oth_sample_step):
        Policy.act (model.py:60-99) over every board's possible_moves followed by
        OthelloBaseEnv.step (othello.py:412-462), bit-identical to the two calls.
        Returns (actions int32, log_probs, entropy, rewards int32, dones bool).
        Outputs may be given to be written in place: `actions` / `rewards` int32 (E,),
        `dones` uint8 (E,), and `log_probs` / `entropy` as float32 (E,) tensors
        instead of True.  observe: an observation layout ('make_state', the
        learners' next input (util.py:48-74), 'board', ...): the stepped boards'
        observation from the same launch (oth_sample_step_observe), into `obs` if
        given or a new `obs_dtype` tensor, appended as a sixth value."""
        x, uniforms = self._sampler_inputs(logits, uniforms)
        acts = self._out(actions, torch.int32, "actions")
        lp = self._out(log_probs, torch.float32, "log_probs")
        ent = self._out(entropy, torch.float32, "entropy")
        r = self._out(rewards, torch.int32, "rewards")
        d = self._out(dones, torch.uint8, "dones")
        mode = (L.OTH_MASKED_MODE if deterministic else L.OTH_MASKED_SAMPLE) | \
            (L.OTH_MASKED_FULL_ENTROPY if full_entropy else 0)
        if observe is None:
            L.check(self._lib.oth_sample_step(self._h, _ptr(x), x.stride(0), _ptr(uniforms), self._sample_calls,
                                              mode, _ptr(acts), _ptr(lp), _ptr(ent), _ptr(r), _ptr(d),
                                              self._stream()), "oth_sample_step")
        else:
            lay, o = self._obs_out(observe, obs_dtype, obs)
            L.check(self._lib.oth_sample_step_observe(self._h, _ptr(x), x.stride(0), _ptr(uniforms),
                                                      self._sample_calls, mode, _ptr(acts), _ptr(lp), _ptr(ent),
                                                      _ptr(r), _ptr(d), lay, _DTYPES[o.dtype], _ptr(o),
                                                      self._stream()), "oth_sample_step_observe")
        self._sample_calls += 1
        res = (acts, lp, ent, r, (d.view(torch.bool) if d is not None else None))
        return res if observe is None else res + (o,)

    @property
    def sample_counter(self):
        """Philox counter of the next eager sample_actions call (purpose 3)."""
        return self._sample_calls

    @sample_counter.setter
    def sample_counter(self, v):
        self._sample_calls = int(v)

    @staticmethod
    def graph_counter_base(slot):
        """First counter of graph region `slot`'s range (ply and sample counters)."""
        return int(slot) << L.OTH_GRAPH_COUNTER_SHIFT

    def graph_offsets(self, slot):
        """(ply, sample) offsets graph region `slot`'s replays have consumed;
        synchronises the device, so never call it during a capture."""
        _no_capture("graph_offsets")
        out = (ctypes.c_uint64 * 2)()
        L.check(self._lib.oth_graph_offsets(self._h, int(slot), out), "oth_graph_offsets")
        return int(out[0]), int(out[1])

    @contextlib.contextmanager
    def graph_region(self):
        """Wrap the calls captured into a HIP graph (enter it INSIDE
        `torch.cuda.graph`).  The region owns a counter range of its own
        (oth_graph_begin: ply and sample counters from slot << 40), and on exit
        enqueues the advance of its device offsets by what the region consumed,
        so replay r draws counters base + r*d .. base + r*d + d - 1: fresh
        Philox numbers every replay (random openings, device opponents,
        sample_actions without uniforms), disjoint from eager calls and from
        every other region of this handle.  Yields the slot.  A region that
        fails gives its slot back; a captured graph keeps it until
        release_graph_slot(slot) (call it when the graph is dropped).

            with torch.cuda.graph(g), env.graph_region() as slot:
                for k in range(K): env.step(env.sample_actions(actor(obs))[0]); ...
        """
        if not torch.cuda.is_current_stream_capturing():
            raise RuntimeError("graph_region must be entered inside torch.cuda.graph(...) "
                               "(with torch.cuda.graph(g), env.graph_region(): ...)")
        slot = ctypes.c_int32()
        L.check(self._lib.oth_graph_begin(self._h, ctypes.byref(slot)), "oth_graph_begin")
        k = int(slot.value)
        smp0, self._sample_calls = self._sample_calls, self.graph_counter_base(k)
        self._region_resets = 0
        ok = False
        try:
            yield k
            ok = True
        finally:
            capturing = torch.cuda.is_current_stream_capturing()
            d_smp = self._sample_calls - self.graph_counter_base(k)
            self._sample_calls = smp0
            d_ply = ctypes.c_uint64()
            rc = self._lib.oth_graph_end(self._h, d_smp, int(capturing), ctypes.byref(d_ply), self._stream())
            resets, self._region_resets = self._region_resets, None
            try:
                if ok:
                    L.check(rc, "oth_graph_end")
                    if not capturing:
                        raise RuntimeError("the capture ended inside graph_region: enter graph_region inside "
                                           "torch.cuda.graph(...), not around it")
                    if resets and self.initial_rand_steps > 0 and d_ply.value == 0:
                        raise RuntimeError("this graph region only resets boards with random openings: every "
                                           "replay would draw the same openings; capture at least one ply with "
                                           "the reset")
            except BaseException:
                ok = False
                raise
            finally:
                if not ok:  # no usable graph: the slot goes back
                    self._lib.oth_graph_release(self._h, k)

    def release_graph_slot(self, slot):
        """Give a graph region's counter slot back once its graph is dropped
        (oth_graph_release); the slot's offsets are kept, so a later region on
        it still draws counters no earlier replay drew."""
        L.check(self._lib.oth_graph_release(self._h, int(slot)), "oth_graph_release")

    def state_dict(self):
        """Boards, meta, possible_moves and the eager counters (host values).
        Graph regions keep their own counter ranges and are not part of it."""
        _no_capture("state_dict")
        b, m, lg = self.get_state()
        return {"boards": b, "meta": m, "legal": lg, "ply_counter": self.ply_counter,
                "sample_calls": self._sample_calls, "playout_calls": self._playout_calls,
                "board_size": self.board_size,
                "num_envs": self.num_envs}

    def load_state_dict(self, sd):
        """Restore a state_dict.  Graphs captured on this handle stay valid and
        keep drawing from their own counter ranges (nothing is zeroed)."""
        _no_capture("load_state_dict")
        if sd["board_size"] != self.board_size or sd["num_envs"] != self.num_envs:
            raise ValueError("state_dict shape does not match this env")
        self.set_state(sd["boards"], sd["meta"], sd["legal"])
        self.ply_counter = sd["ply_counter"]
        self._sample_calls = int(sd.get("sample_calls", 0))
        self._playout_calls = int(sd.get("playout_calls", 0))

    # decoded views of the meta word
    def player_turn(self):
        b, m, _ = self.get_state()
        return torch.where((m & 1) != 0, WHITE_DISK, BLACK_DISK)

    def terminated(self):
        _, m, _ = self.get_state()
        return ((m >> 1) & 1) != 0

    def winner(self):
        _, m, _ = self.get_state()
        w = (m >> 2) & 3
        return torch.where(w == 1, WHITE_DISK, torch.where(w == 2, BLACK_DISK, NO_DISK))


def _numel(shape):
    k = 1
    for x in shape:
        k *= x
    return k


def _no_capture(what):
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("%s synchronises the device and cannot run during a HIP-graph capture" % what)


def _int8_weights(weights, n=None):
    """weights checked as VecOthelloEnv.search takes them: an integer tensor or
    array that fits int8, of shape (N, N) or (N*N,) (N = n, or any board size
    when n is None); returns it as an int8 host or device tensor."""
    w = torch.as_tensor(weights)
    if w.is_floating_point() or w.is_complex() or w.dtype == torch.bool:
        raise ValueError("weights must be integers")
    if n is None:
        side = w.shape[0] if w.dim() == 2 else next((k for k in range(4, 17) if k * k == w.numel()), 0)
    else:
        side = n
    if w.numel() != side * side or w.dim() not in (1, 2) or (w.dim() == 2 and w.shape[0] != side) or \
            not 4 <= side <= 16:
        raise ValueError("weights must have shape (N, N) or (N*N,)")
    if w.dtype != torch.int8:
        if int(w.min()) < -128 or int(w.max()) > 127:
            raise ValueError("weights must fit int8")
        w = w.to(torch.int8)
    return w


class SearchConfig(object):
    """A search as a player (struct oth_search_policy): the move of a board with
    e empty squares is oth_search's `best` at depth e when e <= endgame_empties
    (every line then reaches a game end: the exact move), else at `depth`; where
    the search runs over max_nodes (per root move) GreedyPolicy moves and the ply
    counts as a fallback.  weights / mobility / terminal are VecOthelloEnv.search's
    (None: default_search_weights(N)), checked here as there.  Used by
    VecOthelloEnv.play_search and as `opponent` of reset_vs / step_vs.  The int8
    weights are cached per device and board size, so a captured call copies nothing."""

    def __init__(self, depth=4, weights=None, mobility=0, terminal=64, endgame_empties=0, max_nodes=1 << 22):
        for name, v, lo, hi in (("depth", depth, 1, L.OTH_SEARCH_MAX_DEPTH), ("mobility", mobility, -127, 127),
                                ("terminal", terminal, 1, 32767),
                                ("endgame_empties", endgame_empties, 0, L.OTH_SEARCH_MAX_DEPTH),
                                ("max_nodes", max_nodes, 1, 2 ** 32 - 1)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError("%s must be an integer" % name)
            if not lo <= int(v) <= hi:
                raise ValueError("%s must be in [%d, %d]" % (name, lo, hi))
        self.depth, self.mobility, self.terminal = int(depth), int(mobility), int(terminal)
        self.endgame_empties, self.max_nodes = int(endgame_empties), int(max_nodes)
        self.weights = None if weights is None else _int8_weights(weights).clone()
        self._cache = {}  # (device, N) -> (device weights, OthSearchPolicy)

    def _policy(self, env):
        """The struct for env's device and board size (built once, kept alive here)."""
        key = (str(env.device), env.board_size)
        hit = self._cache.get(key)
        if hit is None:
            if self.weights is None:
                w = env._search_weights(None)
            else:
                w = env._search_weights(self.weights)
            pol = L.OthSearchPolicy(w.data_ptr(), self.depth, self.mobility, self.terminal, self.endgame_empties,
                                    self.max_nodes)
            hit = self._cache[key] = (w, pol)
        return hit[1]

    def __repr__(self):
        return "SearchConfig(depth=%d, weights=%s, mobility=%d, terminal=%d, endgame_empties=%d, max_nodes=%d)" % (
            self.depth, "None" if self.weights is None else "<%d squares>" % self.weights.numel(), self.mobility,
            self.terminal, self.endgame_empties, self.max_nodes)


def default_search_weights(n):
    """The square weights VecOthelloEnv.search uses when it is given none: an int8
    (n, n) tensor on the host, by square class -- corner 100, X-square (a corner's
    diagonal neighbour) -50, C-square (a corner's orthogonal neighbour) -20, any
    other edge square 10, the rest 0; where the classes overlap on small boards
    the precedence is corner > X > C > edge.  A conventional shape, not a tuned
    table.  Measured (tools/arena.py; 16,384 8x8 games per
    pairing and colour, up to 10 random opening plies, the last 10 squares exact):
    SearchConfig(depth=1) wins 92-99 % of its games against the random, greedy and
    MaxiMin-3 movers, depth 4 wins 98-99.6 %; depth 4 beats depth 1 in 90 % of the
    games as either colour, and depth 3 in 64 % as black but in 44 % as white."""
    n = int(n)
    w = torch.zeros(n, n, dtype=torch.int8)
    w[0, :] = w[-1, :] = 10
    w[:, 0] = w[:, -1] = 10
    for r, dr in ((0, 1), (n - 1, -1)):
        for c, dc in ((0, 1), (n - 1, -1)):
            w[r + dr, c] = w[r, c + dc] = -20
    for r, dr in ((0, 1), (n - 1, -1)):
        for c, dc in ((0, 1), (n - 1, -1)):
            w[r + dr, c + dc] = -50
    for r in (0, n - 1):
        for c in (0, n - 1):
            w[r, c] = 100
    return w


def legal_moves(board_size, mover, opponent):
    """Stateless get_possible_actions(board) (othello.py:313-343) on canonical
    boards given as (n, W) int64 mover / opponent masks on a GPU."""
    lib = L.load()
    mover = mover.contiguous()
    opponent = opponent.to(mover.device).contiguous()
    out = torch.empty_like(mover)
    stream = ctypes.c_void_p(torch.cuda.current_stream(mover.device).cuda_stream)
    L.check(lib.oth_legal_moves(int(board_size), int(mover.shape[0]), _ptr(mover), _ptr(opponent), _ptr(out),
                                stream), "oth_legal_moves")
    return out


def symmetry_masks(board_size, sym, masks):
    """Stateless oth_symmetry_masks: masks int64 (n, planes, W) or (n, W) on a GPU, each
    row's planes under the board symmetry sym[i] & 7 (uint8 (n,)): bit sigma_s(a) of the
    result is bit a of the input (symmetry_permutations has sigma)."""
    lib = L.load()
    m = masks.contiguous()
    n = int(m.shape[0])
    planes = int(m.numel() // (n * nwords(max(4, int(board_size))))) if n else 0
    sm = sym.to(device=m.device, dtype=torch.uint8).contiguous()
    if sm.numel() != n:
        raise ValueError("sym must have %d elements" % n)
    out = torch.empty_like(m)
    stream = ctypes.c_void_p(torch.cuda.current_stream(m.device).cuda_stream)
    with torch.cuda.device(m.device):
        L.check(lib.oth_symmetry_masks(int(board_size), n, planes, _ptr(sm), _ptr(m), _ptr(out), stream),
                "oth_symmetry_masks")
    return out


def symmetry_permutations(n):
    """int64 (8, N*N) on the host: [s][a] = sigma_s(a), the square that square a = (r, c)
    goes to under symmetry s of the replay store -- (r, c) transposed if s & 1, then the
    row mirrored if s & 2, then the column if s & 4.  For visits v of a position and
    logits l of its image under s: v_image[sigma[s]] = v, and l[sigma[s]] maps the
    network's logits back to the position's own squares."""
    n = int(n)
    out = torch.empty(8, n * n, dtype=torch.int64)
    for s in range(8):
        for a in range(n * n):
            r, c = divmod(a, n)
            if s & 1:
                r, c = c, r
            if s & 2:
                r = n - 1 - r
            if s & 4:
                c = n - 1 - c
            out[s, a] = r * n + c
    return out
