"""oth_puct_pick and oth_puct_reroot without a GPU: the argument checks, which come
with nothing launched, the ctypes signatures and the Python surface."""
import ctypes
import inspect
import struct

import pytest

from test_puct_capi_cpu import lib, on_a_thread  # noqa: F401


def test_argument_checks_without_gpu(lib):
    from gymothelloenv_amd import _lib as L
    out = (ctypes.c_int32 * 64)()
    arr = ctypes.cast(out, ctypes.c_void_p)
    wsbuf = (ctypes.c_uint64 * 8)()
    ws = ctypes.cast(wsbuf, ctypes.c_void_p)
    # a block that holds only n_envs = 4, board_size = 8 and W = 1 stands in for a handle
    # (tests/test_puct_capi_cpu.py); only rejected calls are made with it
    blank = ctypes.create_string_buffer(struct.pack("<iii", 4, 8, 1), 512)
    h = ctypes.cast(blank, ctypes.c_void_p)
    big = 1 << 40
    need = ctypes.c_uint64(0)
    assert lib.oth_puct_workspace_bytes(8, 4, 4096, ctypes.byref(need)) == 0

    def params(c_puct=320, max_tree_nodes=4096):
        return L.OthPuctParams(c_puct, max_tree_nodes)

    def leaves(layout, dtype, obs=arr):
        return L.OthPuctLeaves(None, None, None, None, obs, layout, dtype)

    ok = params()

    def pick(env, p, wsp=ws, nbytes=big, actions=arr):
        return (lib.oth_puct_pick, (env, None if p is None else ctypes.byref(p), wsp, nbytes, arr, 1, 2, 3, actions,
                                    None))

    def reroot(env, p, wsp=ws, nbytes=big, actions=arr, lv=None):
        return (lib.oth_puct_reroot, (env, None if p is None else ctypes.byref(p), wsp, nbytes, actions, arr, arr,
                                      None if lv is None else ctypes.byref(lv), None))

    cases = []
    for name, call in (("pick", pick), ("reroot", reroot)):
        cases += [
            (name + ": NULL actions", call(None, ok, actions=None), b"actions"),
            (name + ": NULL params", call(None, None), b"params"),
            (name + ": NULL workspace", call(None, ok, wsp=None), b"workspace"),
            (name + ": c_puct = -1", call(None, params(c_puct=-1)), b"c_puct"),
            (name + ": c_puct = 65536", call(None, params(c_puct=65536)), b"c_puct"),
            (name + ": max_tree_nodes = 15", call(None, params(max_tree_nodes=15)), b"max_tree_nodes"),
            (name + ": max_tree_nodes = 2**24 + 1", call(None, params(max_tree_nodes=(1 << 24) + 1)),
             b"max_tree_nodes"),
            (name + ": misaligned workspace", call(None, ok, wsp=ctypes.c_void_p(ws.value + 4)), b"workspace"),
            (name + ": NULL handle", call(None, ok), b"oth_env"),
            (name + ": max_tree_nodes below N*N", call(h, params(max_tree_nodes=63)), b"max_tree_nodes"),
            (name + ": workspace_bytes too small", call(h, ok, nbytes=need.value - 1), b"workspace_bytes"),
        ]
    cases += [
        ("reroot: layout = 5", reroot(None, ok, lv=leaves(5, 0)), b"layout"),
        ("reroot: dtype = 6", reroot(None, ok, lv=leaves(2, 6)), b"dtype"),
        ("reroot: no obs", reroot(None, ok, lv=leaves(99, 99, obs=None)), b"oth_env"),
    ]

    def run():
        return [(what, fn(*args), lib.oth_last_error(), word) for what, (fn, args), word in cases]

    seen = on_a_thread(run)
    assert len(seen) == len(cases)
    for what, rc, msg, word in seen:
        assert rc == -1, what
        assert word in msg, (what, msg)
    assert list(out) == [0] * 64 and list(wsbuf) == [0] * 8  # nothing was written


def test_signatures(lib):
    from gymothelloenv_amd import _lib as L
    P, I32, U32, U64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64
    assert L.SIGNATURES["oth_puct_pick"] == (I32, [P, P, P, U64, P, U64, U32, U64, P, P])
    assert L.SIGNATURES["oth_puct_reroot"] == (I32, [P, P, P, U64, P, P, P, P, P])
    for name in ("oth_puct_pick", "oth_puct_reroot"):
        fn = getattr(lib, name)
        assert fn.restype is I32 and list(fn.argtypes) == L.SIGNATURES[name][1]
    # the workspace is the search's own: its size did not change for the re-root
    b = ctypes.c_uint64(0)
    assert lib.oth_puct_workspace_bytes(8, 9, 4096, ctypes.byref(b)) == 0
    assert b.value == 8 * (2 + 2 * 9 + 3 * 9 + 3 + 9 * 4096 * 7)


def test_python_surface():
    import gymothelloenv_amd as g
    from gymothelloenv_amd import vec_env
    assert g.PuctPlay is vec_env.PuctPlay
    assert vec_env.PuctPlay._fields == ("actions", "visits", "rewards", "dones", "kept")

    def defaults(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()][1:]

    V = vec_env.VecOthelloEnv
    assert defaults(V.puct_pick) == [("sample", None), ("seed", None), ("counter", None)]
    assert defaults(V.puct_reroot) == [("actions", inspect.Parameter.empty), ("root_priors", None), ("kept", False)]
    sig = inspect.signature(V.puct_play).parameters
    assert list(sig)[1:] == ["evaluate", "simulations", "sample", "begin_kw"] and sig["sample"].default is None
    assert sig["begin_kw"].kind is inspect.Parameter.VAR_KEYWORD
    assert isinstance(V.puct_pick_counter, property) and V.puct_pick_counter.fset is not None
    assert "-1" in V.puct_play.__doc__ and "invalid-move path" in V.puct_play.__doc__
