"""Loader for the in-tree HIP library liboth_mi355x.so (C ABI: include/othello_mi355x.h).

There is no CPU fallback: if the library is missing or no GPU is visible, the
product classes raise.  `torch` is imported first so that the library's
`libamdhip64.so.7` dependency resolves to the HIP runtime torch already
loaded -- one runtime per process, so torch streams and tensor pointers are
valid arguments.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "liboth_mi355x.so"
LIB_PATH = os.path.join(HERE, LIB_NAME)

OTH_OK = 0
OTH_SUDDEN_DEATH = 1
OTH_DISK_REWARD = 2
OTH_AUTO_RESET = 4
OTH_POLICY_RANDOM = 0
OTH_POLICY_GREEDY = 1
OTH_POLICY_MAXIMIN1 = 2
OTH_POLICY_MAXIMIN2 = 3
OTH_POLICY_MAXIMIN3 = 4
OTH_MAXIMIN_MAX_DEPTH = 10


def OTH_POLICY_MAXIMIN(d):
    return OTH_POLICY_MAXIMIN1 + int(d) - 1
OTH_OBS_BOARD = 0
OTH_OBS_BOARD_LEGAL = 1
OTH_OBS_MAKE_STATE = 2
OTH_OBS_ABSOLUTE = 3
OTH_OBS_LEGAL = 4
OTH_I8, OTH_I32, OTH_I64, OTH_F32, OTH_F64, OTH_BF16 = range(6)
OTH_MASKED_SAMPLE, OTH_MASKED_MODE, OTH_MASKED_EVAL = range(3)
OTH_MASKED_FULL_ENTROPY = 4
OTH_PLAYOUT_ROOT, OTH_PLAYOUT_MOVES = 0, 1  # oth_playouts modes
OTH_PLAYOUTS_MAX = 65536
OTH_SOLVE_MAX_EMPTIES = 14  # oth_solve
OTH_SOLVE_NO_VALUE = -32768
OTH_SOLVE_EXACT, OTH_SOLVE_TERMINATED, OTH_SOLVE_SKIPPED, OTH_SOLVE_NO_MOVE, OTH_SOLVE_ABORTED = range(5)
OTH_SEARCH_MAX_DEPTH = 14  # oth_search
OTH_SEARCH_NO_VALUE = -2 ** 31
OTH_SEARCH_DONE, OTH_SEARCH_TERMINATED, OTH_SEARCH_NO_MOVE, OTH_SEARCH_ABORTED = 0, 1, 3, 4
OTH_MCTS_MAX_ITERATIONS, OTH_MCTS_MAX_PLAYOUTS, OTH_MCTS_MAX_C = 65535, 64, 65535  # oth_mcts
OTH_MCTS_MAX_TREE_NODES = 1 << 24
OTH_MCTS_DONE, OTH_MCTS_TERMINATED, OTH_MCTS_NO_MOVE = 0, 1, 3
OTH_PUCT_VALUE_ONE, OTH_PUCT_PRIOR_MAX, OTH_PUCT_MAX_C = 32768, 65535, 65535  # oth_puct_*
OTH_PUCT_MAX_TREE_NODES, OTH_PUCT_MAX_SIMS = 1 << 24, (1 << 24) - 1
OTH_PUCT_LEAF_NONE, OTH_PUCT_LEAF_EXPAND, OTH_PUCT_LEAF_VALUE, OTH_PUCT_LEAF_TERMINAL = range(4)
OTH_PUCT_MAX_LEAVES = 64  # oth_puct_*_batch
OTH_NOISE_TABLE, OTH_NOISE_G_MAX = 4096, 1 << 24  # oth_puct_noise
OTH_REPLAY_MAX_HORIZON, OTH_REPLAY_MAX_ROWS, OTH_REPLAY_MAX_BATCH = 65536, 1 << 24, 1 << 20  # oth_replay_*
OTH_REPLAY_EMPTY, OTH_REPLAY_OPEN, OTH_REPLAY_LABELLED = range(3)
OTH_NET_MAX_LAYERS, OTH_NET_MAX_WIDTH, OTH_NET_MAX_SHIFT = 4, 512, 24  # oth_net_*
OTH_NET_BIAS_MAX, OTH_NET_MAX_ROWS = 1 << 30, 1 << 24
OTH_NET_SAMPLE_DISCS_MAX = 257
OTH_CNET_MAX_BLOCKS = 8  # oth_cnet_*
OTH_NTUPLE_MAX_TUPLES, OTH_NTUPLE_MAX_LENGTH, OTH_NTUPLE_MAX_ROWS = 32, 8, 1 << 24  # oth_ntuple_*
OTH_NTUPLE_MAX_RATE, OTH_NTUPLE_MAX_RATE_SHIFT = 1 << 24, 40
OTH_NTUPLE_EXPLORE_ONE = 65536  # oth_ntuple_policy.explore: epsilon in 1 / 65536
OTH_GRAPH_SLOTS = 64
OTH_GRAPH_COUNTER_SHIFT = 40

OTH_RECORD_MAX_WORDS = 4
OTH_RECORD_MAX_SQUARES = 256
OTH_RECORD_GREEDY = 2  # oth_step_sync's `step` bit: the record carries GreedyPolicy's move
OTH_RECORD_NO_GREEDY = -2


class OthRecord(ctypes.Structure):
    """struct oth_record (include/othello_mi355x.h): one board as oth_step_sync
    leaves it in the handle's mapped host buffer."""
    _fields_ = [("black", ctypes.c_uint64 * OTH_RECORD_MAX_WORDS),
                ("white", ctypes.c_uint64 * OTH_RECORD_MAX_WORDS),
                ("legal", ctypes.c_uint64 * OTH_RECORD_MAX_WORDS),
                ("seq", ctypes.c_uint32),
                ("meta", ctypes.c_uint16),
                ("done", ctypes.c_uint8),
                ("planes", ctypes.c_uint8),
                ("reward", ctypes.c_int32),
                ("white_cnt", ctypes.c_int32),
                ("black_cnt", ctypes.c_int32),
                ("greedy", ctypes.c_int32),
                ("obs", ctypes.c_int8 * (2 * OTH_RECORD_MAX_SQUARES)),
                ("board_state", ctypes.c_int8 * OTH_RECORD_MAX_SQUARES)]


class OthSearchPolicy(ctypes.Structure):
    """struct oth_search_policy (include/othello_mi355x.h): one colour's search
    configuration, host memory read during the call; `weights` is a device address."""
    _fields_ = [("weights", ctypes.c_void_p),
                ("depth", ctypes.c_int32),
                ("mobility_weight", ctypes.c_int32),
                ("terminal_weight", ctypes.c_int32),
                ("endgame_empties", ctypes.c_int32),
                ("max_nodes", ctypes.c_uint64)]


class OthMctsParams(ctypes.Structure):
    """struct oth_mcts_params (include/othello_mi355x.h): host memory read during the call."""
    _fields_ = [("iterations", ctypes.c_int32),
                ("playouts", ctypes.c_int32),
                ("c_explore", ctypes.c_int32),
                ("max_tree_nodes", ctypes.c_int32),
                ("seed", ctypes.c_uint64),
                ("id_key", ctypes.c_uint32),
                ("counter", ctypes.c_uint64)]


class OthPuctParams(ctypes.Structure):
    """struct oth_puct_params (include/othello_mi355x.h): host memory read during the call."""
    _fields_ = [("c_puct", ctypes.c_int32),
                ("max_tree_nodes", ctypes.c_int32)]


class OthPuctLeaves(ctypes.Structure):
    """struct oth_puct_leaves (include/othello_mi355x.h): host memory holding device
    addresses, each may be NULL."""
    _fields_ = [("kind", ctypes.c_void_p),
                ("boards", ctypes.c_void_p),
                ("meta", ctypes.c_void_p),
                ("legal", ctypes.c_void_p),
                ("obs", ctypes.c_void_p),
                ("layout", ctypes.c_int32),
                ("dtype", ctypes.c_int32)]


class OthReplayBatch(ctypes.Structure):
    """struct oth_replay_batch (include/othello_mi355x.h): host memory holding device
    addresses, each may be NULL."""
    _fields_ = [("state", ctypes.c_void_p),
                ("boards", ctypes.c_void_p),
                ("meta", ctypes.c_void_p),
                ("legal", ctypes.c_void_p),
                ("visits", ctypes.c_void_p),
                ("outcome", ctypes.c_void_p),
                ("obs", ctypes.c_void_p),
                ("layout", ctypes.c_int32),
                ("dtype", ctypes.c_int32),
                ("rows", ctypes.c_void_p),
                ("sym", ctypes.c_void_p)]


class OthNetParams(ctypes.Structure):
    """struct oth_net_params (include/othello_mi355x.h): host memory read during the call."""
    _fields_ = [("layers", ctypes.c_int32),
                ("width", ctypes.c_int32),
                ("shift", ctypes.c_int32 * 4),
                ("policy_shift", ctypes.c_int32),
                ("value_shift", ctypes.c_int32)]


class OthCnetParams(ctypes.Structure):
    """struct oth_cnet_params (include/othello_mi355x.h): host memory read during the call."""
    _fields_ = [("channels", ctypes.c_int32),
                ("blocks", ctypes.c_int32),
                ("shift_stem", ctypes.c_int32),
                ("shift", ctypes.c_int32 * 16),
                ("shift_head", ctypes.c_int32),
                ("policy_shift", ctypes.c_int32),
                ("value_shift", ctypes.c_int32)]


class OthNtupleParams(ctypes.Structure):
    """struct oth_ntuple_params (include/othello_mi355x.h): host memory read during the call."""
    _fields_ = [("tuples", ctypes.c_int32),
                ("length", ctypes.c_int32 * 32),
                ("squares", (ctypes.c_int32 * 8) * 32),
                ("value_shift", ctypes.c_int32)]


class OthNetPolicy(ctypes.Structure):
    """struct oth_net_policy (include/othello_mi355x.h): one colour's network as a
    player, host memory read during the call; `blob` is a device address."""
    _fields_ = [("params", OthNetParams),
                ("blob", ctypes.c_void_p),
                ("blob_bytes", ctypes.c_uint64),
                ("sample_discs", ctypes.c_int32)]


class OthCnetPolicy(ctypes.Structure):
    """struct oth_cnet_policy (include/othello_mi355x.h): one colour's convolutional
    network as a player, host memory read during the call; `blob` is a device address."""
    _fields_ = [("params", OthCnetParams),
                ("blob", ctypes.c_void_p),
                ("blob_bytes", ctypes.c_uint64),
                ("sample_discs", ctypes.c_int32)]


class OthNtuplePolicy(ctypes.Structure):
    """struct oth_ntuple_policy (include/othello_mi355x.h): one colour's n-tuple network
    as a player, host memory read during the call; `plan` and `weights` are device
    addresses."""
    _fields_ = [("params", OthNtupleParams),
                ("plan", ctypes.c_void_p),
                ("plan_bytes", ctypes.c_uint64),
                ("weights", ctypes.c_void_p),
                ("weight_count", ctypes.c_uint64),
                ("depth", ctypes.c_int32),
                ("terminal_weight", ctypes.c_int32),
                ("endgame_empties", ctypes.c_int32),
                ("explore", ctypes.c_int32),
                ("max_nodes", ctypes.c_uint64)]


class OthNtupleTd(ctypes.Structure):
    """struct oth_ntuple_td (include/othello_mi355x.h): host memory holding device
    addresses, all required."""
    _fields_ = [("boards", ctypes.c_void_p),
                ("meta", ctypes.c_void_p),
                ("targets", ctypes.c_void_p),
                ("learn", ctypes.c_void_p)]


# every symbol include/othello_mi355x.h declares: (restype, argtypes)
_P = ctypes.c_void_p
_I32, _U32, _U64, _I64 = ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64
SIGNATURES = {
    "oth_create": (_I32, [_I32, _I32, _U32, _U64, _U32, _I32, _I32, ctypes.POINTER(_P)]),
    "oth_destroy": (_I32, [_P]),
    "oth_reset": (_I32, [_P, _P, _P]),
    "oth_step": (_I32, [_P, _P, _P, _P, _P]),
    "oth_step_observe": (_I32, [_P, _P, _P, _P, _I32, _I32, _P, _P]),
    "oth_step_sync": (_I32, [_P, _I32, _I32, _I32, _I32, ctypes.POINTER(_P), _P]),
    "oth_step_policy": (_I32, [_P, _I32, _I32, _P, _P, _P, _P]),
    "oth_playouts": (_I32, [_P, _I32, _I32, _U64, _U32, _U64, _P, _P, _P, _P]),
    "oth_solve": (_I32, [_P, _I32, _U64, _P, _P, _P, _P, _P, _P]),
    "oth_search": (_I32, [_P, _I32, _P, _I32, _I32, _U64, _P, _P, _P, _P, _P, _P]),
    "oth_mcts_workspace_bytes": (_I32, [_I32, _I32, _I32, _P]),
    "oth_mcts": (_I32, [_P, _P, _P, _U64, _P, _P, _P, _P, _P, _P]),
    "oth_puct_workspace_bytes": (_I32, [_I32, _I32, _I32, _P]),
    "oth_puct_begin": (_I32, [_P, _P, _P, _U64, _P, _P]),
    "oth_puct_advance": (_I32, [_P, _P, _P, _U64, _P, _P, _I32, _P, _P]),
    "oth_puct_result": (_I32, [_P, _P, _P, _U64, _P, _P, _P, _P, _P, _P]),
    "oth_puct_pick": (_I32, [_P, _P, _P, _U64, _P, _U64, _U32, _U64, _P, _P]),
    "oth_puct_reroot": (_I32, [_P, _P, _P, _U64, _P, _P, _P, _P, _P]),
    "oth_puct_noise": (_I32, [_P, _I32, _P, _P, _P, _P, _I32, _P, _U64, _U32, _U64, _P]),
    "oth_puct_batch_workspace_bytes": (_I32, [_I32, _I32, _I32, _I32, _P]),
    "oth_puct_begin_batch": (_I32, [_P, _P, _I32, _P, _U64, _P, _P]),
    "oth_puct_advance_batch": (_I32, [_P, _P, _I32, _P, _U64, _P, _P, _I32, _P, _P]),
    "oth_puct_reroot_batch": (_I32, [_P, _P, _I32, _P, _U64, _P, _P, _P, _I32, _P, _P]),
    "oth_replay_workspace_bytes": (_I32, [_I32, _I32, _I32, _I32, _P]),
    "oth_replay_begin": (_I32, [_P, _I32, _I32, _P, _U64, _P]),
    "oth_replay_append": (_I32, [_P, _I32, _I32, _P, _U64, _P, _P, _P]),
    "oth_replay_label": (_I32, [_P, _I32, _I32, _P, _U64, _P, _P, _P]),
    "oth_replay_counts": (_I32, [_P, _I32, _I32, _P, _U64, _P, _P]),
    "oth_replay_gather": (_I32, [_P, _I32, _I32, _P, _U64, _I32, _P, _P, _P, _P]),
    "oth_replay_sample": (_I32, [_P, _I32, _I32, _P, _U64, _I32, _I32, _U64, _U32, _U64, _P, _P]),
    "oth_symmetry_masks": (_I32, [_I32, _I32, _I32, _P, _P, _P, _P]),
    "oth_net_blob_bytes": (_I32, [_I32, _P, _P]),
    "oth_net_pack": (_I32, [_I32, _P, _P, _P, _P, _U64]),
    "oth_net_eval": (_I32, [_I32, _I32, _P, _P, _U64, _P, _P, _P, _P, _P, _P, _P]),
    "oth_cnet_blob_bytes": (_I32, [_I32, _P, _P]),
    "oth_cnet_pack": (_I32, [_I32, _P, _P, _P, _P, _U64]),
    "oth_cnet_eval": (_I32, [_I32, _I32, _P, _P, _U64, _P, _P, _P, _P, _P, _P, _P]),
    "oth_ntuple_weight_count": (_I32, [_I32, _P, _P]),
    "oth_ntuple_plan_bytes": (_I32, [_I32, _P, _P]),
    "oth_ntuple_plan": (_I32, [_I32, _P, _P, _U64]),
    "oth_ntuple_eval": (_I32, [_I32, _I32, _P, _P, _U64, _P, _U64, _P, _P, _P, _P, _P]),
    "oth_ntuple_update": (_I32, [_I32, _I32, _P, _P, _U64, _P, _U64, _P, _P, _P, _I32, _I32, _P, _P]),
    "oth_search_ntuple": (_I32, [_P, _I32, _P, _P, _U64, _P, _U64, _I32, _U64, _P, _P, _P, _P, _P, _P]),
    "oth_play_search": (_I32, [_P, _P, _P, _I32, _P, _P, _P, _P, _P]),
    "oth_reset_vs_search": (_I32, [_P, _P, _P, _P, _P]),
    "oth_step_vs_search": (_I32, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "oth_play_net": (_I32, [_P, _P, _P, _I32, _P, _P, _P, _P]),
    "oth_reset_vs_net": (_I32, [_P, _P, _P, _P, _P]),
    "oth_step_vs_net": (_I32, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "oth_play_cnet": (_I32, [_P, _P, _P, _I32, _P, _P, _P, _P]),
    "oth_reset_vs_cnet": (_I32, [_P, _P, _P, _P, _P]),
    "oth_step_vs_cnet": (_I32, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "oth_play_ntuple": (_I32, [_P, _P, _P, _I32, _P, _P, _P, _P, _P, _P]),
    "oth_reset_vs_ntuple": (_I32, [_P, _P, _P, _P, _P]),
    "oth_step_vs_ntuple": (_I32, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "oth_ntuple_update_masked": (_I32, [_I32, _I32, _P, _P, _U64, _P, _U64, _P, _P, _P, _P, _I32, _I32, _P, _P]),
    "oth_reset_vs": (_I32, [_P, _I32, _P, _P, _P]),
    "oth_step_vs": (_I32, [_P, _I32, _P, _P, _P, _P, _P, _P]),
    "oth_step_vs_observe": (_I32, [_P, _I32, _P, _P, _P, _P, _P, _I32, _I32, _P, _P]),
    "oth_legal": (_I32, [_P, _P, _P]),
    "oth_legal_moves": (_I32, [_I32, _I32, _P, _P, _P, _P]),
    "oth_greedy_actions": (_I32, [_P, _P, _P]),
    "oth_policy_actions": (_I32, [_P, _I32, _P, _P]),
    "oth_observe": (_I32, [_P, _I32, _I32, _P, _P]),
    "oth_get_state": (_I32, [_P, _P, _P, _P, _P]),
    "oth_set_state": (_I32, [_P, _P, _P, _P, _P]),
    "oth_set_player_turn": (_I32, [_P, _I32, _P, _P]),
    "oth_count_disks": (_I32, [_P, _P, _P]),
    "oth_counts": (_I32, [_P, _P, _I32, _P]),
    "oth_counts_vs": (_I32, [_P, _P, _I32, _P]),
    "oth_masked_sample": (_I32, [_I32, _I32, _P, _I64, _P, _P, _U64, _U32, _U64, _I32, _P, _P, _P, _P]),
    "oth_sample_actions": (_I32, [_P, _P, _I64, _P, _U64, _I32, _P, _P, _P, _P]),
    "oth_sample_step": (_I32, [_P, _P, _I64, _P, _U64, _I32, _P, _P, _P, _P, _P, _P]),
    "oth_sample_step_observe": (_I32, [_P, _P, _I64, _P, _U64, _I32, _P, _P, _P, _P, _P, _I32, _I32, _P, _P]),
    "oth_ply_counter": (_U64, [_P]),
    "oth_set_ply_counter": (_I32, [_P, _U64]),
    "oth_graph_begin": (_I32, [_P, _P]),
    "oth_graph_end": (_I32, [_P, _U64, _I32, _P, _P]),
    "oth_graph_offsets": (_I32, [_P, _I32, _P]),
    "oth_graph_release": (_I32, [_P, _I32]),
    "oth_shape": (_I32, [_P, _P, _P, _P]),
    "oth_last_error": (ctypes.c_char_p, []),
    "oth_version": (ctypes.c_char_p, []),
}

_lib = None


class OthelloLibError(RuntimeError):
    pass


def load(require_gpu=True):
    """Load (once) and return the ctypes handle of liboth_mi355x.so.

    require_gpu=False only loads the library (symbol checks on a CPU host)."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (HIP runtime first: see module docstring)
        if not os.path.exists(LIB_PATH):
            raise OthelloLibError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        from . import build as _build
        have, want = _build.embedded_hash(LIB_PATH), _build.source_hash()
        if have != want:
            raise OthelloLibError(
                "%s was built from other sources (embedded %s, tree %s): rebuild it with "
                "`python -m gymothelloenv_amd.build`" % (LIB_PATH, (have or "none")[:16], want[:16]))
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    if require_gpu:
        import torch
        if not torch.cuda.is_available():
            raise OthelloLibError("no GPU visible: the MI355X Othello engine has no CPU fallback")
    return _lib


def load_path(path):
    """Load another build of the same C ABI (A/B experiments: tools/ab_variants.py)."""
    import torch  # noqa: F401
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)  # an older variant may lack newer entry points
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    return lib


def check(rc, what="", lib=None):
    if rc != OTH_OK:
        msg = (lib or _lib).oth_last_error().decode() if (lib or _lib) is not None else ""
        raise OthelloLibError("%s failed (%d): %s" % (what or "oth call", rc, msg))
    return rc
