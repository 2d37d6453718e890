"""oth_mcts without a GPU: the argument checks, which come with nothing
launched, oth_mcts_workspace_bytes, which needs no handle, and the Python
surface."""
import ctypes
import inspect
import struct
import threading

import pytest


@pytest.fixture(scope="module")
def lib():
    from gymothelloenv_amd import _lib
    from gymothelloenv_amd import build as hb
    if hb.needs_build():
        hb.build()
    return _lib.load(require_gpu=False)


def on_a_thread(fn):
    """oth_last_error is per thread: rejected calls run on a thread of their own, so
    this thread's message (other tests look at it) stays as it was."""
    out = []
    t = threading.Thread(target=lambda: out.append(fn()))
    t.start()
    t.join()
    assert len(out) == 1
    return out[0]


def test_argument_checks_without_gpu(lib):
    from gymothelloenv_amd import _lib as L
    assert (L.OTH_MCTS_DONE, L.OTH_MCTS_TERMINATED, L.OTH_MCTS_NO_MOVE) == (0, 1, 3)
    assert (L.OTH_MCTS_MAX_ITERATIONS, L.OTH_MCTS_MAX_PLAYOUTS, L.OTH_MCTS_MAX_C, L.OTH_MCTS_MAX_TREE_NODES) == (
        65535, 64, 65535, 1 << 24)
    out = (ctypes.c_int32 * 64)()
    vis = ctypes.cast(out, ctypes.c_void_p)
    wsbuf = (ctypes.c_uint64 * 8)()
    ws = ctypes.cast(wsbuf, ctypes.c_void_p)
    # The last checks need the handle's geometry and nothing else of it, so without a GPU
    # (no handle can be created) a block that holds only n_envs = 4, board_size = 8 and
    # W = 1 stands in for one; only rejected calls are made with it.
    blank = ctypes.create_string_buffer(struct.pack("<iii", 4, 8, 1), 512)
    h = ctypes.cast(blank, ctypes.c_void_p)
    big = 1 << 40

    def params(**kw):
        d = dict(iterations=64, playouts=8, c_explore=256, max_tree_nodes=4096, seed=1, id_key=2, counter=3)
        d.update(kw)
        return L.OthMctsParams(**d)

    def call(env, p, wsp=ws, nbytes=big, v=vis):
        return (env, None if p is None else ctypes.byref(p), wsp, nbytes, v, None, None, None, None, None)

    ok = params()
    cases = [
        ("NULL params", call(None, None), b"params"),
        ("NULL workspace", call(None, ok, wsp=None), b"workspace"),
        ("NULL visits", call(None, ok, v=None), b"visits"),
        ("iterations = 0", call(None, params(iterations=0)), b"iterations"),
        ("iterations = 65536", call(None, params(iterations=65536)), b"iterations"),
        ("playouts = 0", call(None, params(playouts=0)), b"playouts"),
        ("playouts = 65", call(None, params(playouts=65)), b"playouts"),
        ("c_explore = -1", call(None, params(c_explore=-1)), b"c_explore"),
        ("c_explore = 65536", call(None, params(c_explore=65536)), b"c_explore"),
        ("max_tree_nodes = 15", call(None, params(max_tree_nodes=15)), b"max_tree_nodes"),
        ("max_tree_nodes = 2**24 + 1", call(None, params(max_tree_nodes=(1 << 24) + 1)), b"max_tree_nodes"),
        ("counter = 2**56", call(None, params(counter=2 ** 56)), b"counter"),
        ("misaligned workspace", call(None, ok, wsp=ctypes.c_void_p(ws.value + 4)), b"workspace"),
        ("NULL handle", call(None, ok), b"oth_env"),
        ("max_tree_nodes below N*N", call(h, params(max_tree_nodes=63)), b"max_tree_nodes"),
        ("workspace_bytes too small", call(h, ok, nbytes=4 * 4096 * 48 - 1), b"workspace_bytes"),
    ]

    def run():
        return [(what, lib.oth_mcts(*args), lib.oth_last_error(), word) for what, args, word in cases]

    seen = on_a_thread(run)
    assert len(seen) == len(cases)
    for what, rc, msg, word in seen:
        assert rc == -1, what
        assert word in msg, (what, msg)
    assert list(out) == [0] * 64 and list(wsbuf) == [0] * 8  # nothing was written


def test_workspace_bytes(lib):
    def size(n, E, T):
        b = ctypes.c_uint64(0)
        rc = lib.oth_mcts_workspace_bytes(n, E, T, ctypes.byref(b))
        return rc, b.value

    def run():
        bad = [(3, 4, 64), (17, 4, 4096), (8, 0, 4096), (8, 4, 63), (8, 4, (1 << 24) + 1), (16, 4, 255)]
        res = [(args, size(*args)[0], lib.oth_last_error()) for args in bad]
        res.append(("NULL bytes", lib.oth_mcts_workspace_bytes(8, 4, 4096, None), lib.oth_last_error()))
        return res

    for what, rc, msg in on_a_thread(run):
        assert rc == -1 and msg, what
    for n in range(4, 17):
        W = (n * n + 63) // 64
        prev = 0
        for E in (1, 2, 9, 65536):
            rc, b = size(n, E, n * n)
            assert rc == 0 and b > prev and b >= E * n * n * 2 * W * 8
            prev = b
        prev = 0
        for T in (n * n, n * n + 1, 4096, 1 << 24):
            rc, b = size(n, 7, T)
            assert rc == 0 and b > prev and b >= 7 * T * 2 * W * 8
            prev = b
    assert size(8, 65536, 1 << 24)[1] >= 65536 * (1 << 24) * 16  # no 32-bit overflow


def test_python_surface():
    import gymothelloenv_amd as g
    from gymothelloenv_amd import policies, vec_env
    assert g.MCTSPolicy is policies.MCTSPolicy and "MCTSPolicy" in policies.__all__
    pol = g.MCTSPolicy()
    assert (pol.iterations, pol.playouts, pol.c, pol.counter) == (256, 8, 1.0, 0)
    for name in ("reset", "get_action", "get_test_action", "seed"):
        assert callable(getattr(pol, name))
    pol.counter = 5
    pol.seed(9)
    assert pol.counter == 0
    sig = inspect.signature(vec_env.VecOthelloEnv.mcts)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [
        ("iterations", inspect.Parameter.empty), ("playouts", 8), ("c", 1.0), ("max_tree_nodes", None),
        ("seed", None), ("id_key", 0), ("counter", None), ("wins2", False), ("best", False), ("tree_nodes", False),
        ("status", False)]
    assert callable(vec_env.VecOthelloEnv.mcts_actions)
