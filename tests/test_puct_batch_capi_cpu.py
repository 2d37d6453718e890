"""oth_puct_begin_batch / _advance_batch / _reroot_batch without a GPU: the argument
checks, which come with nothing launched, oth_puct_batch_workspace_bytes, which
needs no handle, and the Python surface."""
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
    """oth_last_error is per thread: rejected calls run on a thread of their own."""
    out = []
    t = threading.Thread(target=lambda: out.append(fn()))
    t.start()
    t.join()
    assert len(out) == 1
    return out[0]


def test_workspace_bytes(lib):
    from gymothelloenv_amd import _lib as L
    assert L.OTH_PUCT_MAX_LEAVES == 64

    def size(n, E, T, K):
        b = ctypes.c_uint64(0)
        return lib.oth_puct_batch_workspace_bytes(n, E, T, K, ctypes.byref(b)), b.value

    def plain(n, E, T):
        b = ctypes.c_uint64(0)
        assert lib.oth_puct_workspace_bytes(n, E, T, ctypes.byref(b)) == 0
        return b.value

    def run():
        bad = [(3, 4, 64, 4), (17, 4, 4096, 4), (8, 0, 4096, 4), (8, 4, 63, 4), (8, 4, (1 << 24) + 1, 4),
               (8, 4, 4096, 0), (8, 4, 4096, 65), (8, 4, 4096, -1)]
        res = [(args, size(*args), lib.oth_last_error()) for args in bad]
        res.append(("NULL bytes", (lib.oth_puct_batch_workspace_bytes(8, 4, 4096, 4, None), 0), lib.oth_last_error()))
        return res

    for what, (rc, b), msg in on_a_thread(run):
        assert rc == -1 and msg and b == 0, what
    for n in (4, 6, 8, 9, 10, 16):
        W = (n * n + 63) // 64
        for E, T in ((1, n * n), (9, 4096), (70, 512), (65536, n * n), (7, 1 << 24)):
            last = plain(n, E, T)
            for K in (1, 2, 3, 4, 8, 63, 64):
                rc, b = size(n, E, T, K)
                # the plain workspace to an even word, two tags, the E K rows of leaves, a slot word a row
                want = 8 * ((plain(n, E, T) // 8 + 1) // 2 * 2 + 2 + 3 * W * E * K + (E * K + 3) // 4 + E * K)
                assert rc == 0 and b == want and b % 8 == 0, (n, E, T, K)
                assert b > last, "K = 1 is above the plain size, and the size grows with K"
                last = b


def test_argument_checks_without_gpu(lib):
    from gymothelloenv_amd import _lib as L
    out = (ctypes.c_int32 * 64)()
    arr = ctypes.cast(out, ctypes.c_void_p)
    wsbuf = (ctypes.c_uint64 * 8)()
    ws = ctypes.cast(wsbuf, ctypes.c_void_p)
    # the stand-in of tests/test_puct_capi_cpu.py: a block that holds only n_envs = 4, board_size = 8, W = 1
    blank = ctypes.create_string_buffer(struct.pack("<iii", 4, 8, 1), 512)
    h = ctypes.cast(blank, ctypes.c_void_p)
    wide = ctypes.cast(ctypes.create_string_buffer(struct.pack("<iii", 1 << 26, 8, 1), 512), ctypes.c_void_p)
    big = 1 << 50
    need, need_plain = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert lib.oth_puct_batch_workspace_bytes(8, 4, 4096, 4, ctypes.byref(need)) == 0
    assert lib.oth_puct_workspace_bytes(8, 4, 4096, ctypes.byref(need_plain)) == 0

    def params(c_puct=320, max_tree_nodes=4096):
        return L.OthPuctParams(c_puct, max_tree_nodes)

    def leaves(layout, dtype, obs=arr):
        return L.OthPuctLeaves(None, None, None, None, obs, layout, dtype)

    ok = params()

    def ref(x):
        return None if x is None else ctypes.byref(x)

    def begin(env, p, K=4, wsp=ws, nbytes=big, lv=None, lim=5):
        return lib.oth_puct_begin_batch, (env, ref(p), K, wsp, nbytes, ref(lv), None)

    def advance(env, p, K=4, wsp=ws, nbytes=big, priors=arr, values=arr, lv=None, lim=5):
        return lib.oth_puct_advance_batch, (env, ref(p), K, wsp, nbytes, priors, values, lim, ref(lv), None)

    def reroot(env, p, K=4, wsp=ws, nbytes=big, actions=arr, lv=None, lim=5):
        return lib.oth_puct_reroot_batch, (env, ref(p), K, wsp, nbytes, actions, None, None, lim, ref(lv), None)

    cases = []
    for name, call in (("begin", begin), ("advance", advance), ("reroot", reroot)):
        cases += [
            (name + ": NULL params", call(None, None), b"params"),
            (name + ": NULL workspace", call(None, ok, wsp=None), b"workspace"),
            (name + ": c_puct = -1", call(None, params(c_puct=-1)), b"c_puct"),
            (name + ": c_puct = 65536", call(None, params(c_puct=65536)), b"c_puct"),
            (name + ": max_tree_nodes = 15", call(None, params(max_tree_nodes=15)), b"max_tree_nodes"),
            (name + ": max_tree_nodes = 2**24 + 1", call(None, params(max_tree_nodes=(1 << 24) + 1)),
             b"max_tree_nodes"),
            (name + ": misaligned workspace", call(None, ok, wsp=ctypes.c_void_p(ws.value + 4)), b"workspace"),
            (name + ": K = 0", call(None, ok, K=0), b"K must"),
            (name + ": K = 65", call(None, ok, K=65), b"K must"),
            (name + ": K = -4", call(h, ok, K=-4), b"K must"),
            (name + ": layout = 5", call(None, ok, lv=leaves(5, 0)), b"layout"),
            (name + ": dtype = 6", call(None, ok, lv=leaves(2, 6)), b"dtype"),
            (name + ": no obs", call(None, ok, lv=leaves(99, 99, obs=None)), b"oth_env"),
            (name + ": NULL handle", call(None, ok), b"oth_env"),
            (name + ": max_tree_nodes below N*N", call(h, params(max_tree_nodes=63)), b"max_tree_nodes"),
            (name + ": workspace_bytes below the plain size", call(h, ok, nbytes=need_plain.value - 1),
             b"workspace_bytes"),
            (name + ": workspace_bytes of the plain size", call(h, ok, nbytes=need_plain.value),
             b"oth_puct_batch_workspace_bytes"),
            (name + ": workspace_bytes too small", call(h, ok, nbytes=need.value - 1),
             b"oth_puct_batch_workspace_bytes"),
            (name + ": n_envs K above 2^31 - 1", call(wide, ok, K=64), b"rows"),
        ]
    for name, call in (("advance", advance), ("reroot", reroot)):
        cases += [
            (name + ": sim_limit = -1", call(None, ok, lim=-1), b"sim_limit"),
            (name + ": sim_limit = 2^24", call(None, ok, lim=1 << 24), b"sim_limit"),
        ]
    cases += [
        ("advance: NULL priors", advance(None, ok, priors=None), b"priors"),
        ("advance: NULL values", advance(None, ok, values=None), b"values"),
        ("reroot: NULL actions", reroot(None, ok, actions=None), b"actions"),
    ]

    def run():
        return [(what, fn(*args), lib.oth_last_error(), word) for what, (fn, args), word in cases]

    seen = on_a_thread(run)
    assert len(seen) == len(cases)
    for what, rc, msg, word in seen:
        assert rc == -1, what
        assert word in msg, (what, msg)
    assert list(out) == [0] * 64 and list(wsbuf) == [0] * 8  # nothing was written


def test_python_surface():
    import torch

    import gymothelloenv_amd as g
    from gymothelloenv_amd import vec_env

    def defaults(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()][1:]

    V = vec_env.VecOthelloEnv
    empty = inspect.Parameter.empty
    assert defaults(V.puct_begin_batch) == [("leaves_per_board", empty), ("c", 1.25), ("max_tree_nodes", None),
                                            ("layout", "make_state"), ("dtype", torch.float32)]
    assert defaults(V.puct_advance_batch) == [("priors", empty), ("values", empty), ("sim_limit", None)]
    assert defaults(V.puct_reroot_batch) == [("actions", empty), ("root_priors", None), ("kept", False),
                                             ("sim_limit", None)]
    for fn in (V.puct_search, V.puct_play):
        assert "leaves_per_board" in fn.__doc__
    pol = g.PUCTPolicy(leaves_per_board=8)
    assert (pol.simulations, pol.c, pol.leaves_per_board) == (128, 1.25, 8)
    assert g.PUCTPolicy().leaves_per_board == 1
    for bad in (0, 65):
        with pytest.raises(ValueError, match="leaves_per_board"):
            g.PUCTPolicy(leaves_per_board=bad)
