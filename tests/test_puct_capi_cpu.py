"""oth_puct_begin / _advance / _result without a GPU: the argument checks, which
come with nothing launched, oth_puct_workspace_bytes, which needs no handle, and
the Python surface."""
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
    assert (L.OTH_PUCT_VALUE_ONE, L.OTH_PUCT_PRIOR_MAX, L.OTH_PUCT_MAX_C, L.OTH_PUCT_MAX_TREE_NODES,
            L.OTH_PUCT_MAX_SIMS) == (32768, 65535, 65535, 1 << 24, (1 << 24) - 1)
    assert (L.OTH_PUCT_LEAF_NONE, L.OTH_PUCT_LEAF_EXPAND, L.OTH_PUCT_LEAF_VALUE,
            L.OTH_PUCT_LEAF_TERMINAL) == (0, 1, 2, 3)
    assert ctypes.sizeof(L.OthPuctParams) == 8 and ctypes.sizeof(L.OthPuctLeaves) == 48
    out = (ctypes.c_int32 * 64)()
    arr = ctypes.cast(out, ctypes.c_void_p)
    wsbuf = (ctypes.c_uint64 * 8)()
    ws = ctypes.cast(wsbuf, ctypes.c_void_p)
    # The last checks need the handle's geometry and nothing else of it, so without a GPU
    # (no handle can be created) a block that holds only n_envs = 4, board_size = 8 and
    # W = 1 stands in for one; only rejected calls are made with it.
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

    def begin(env, p, wsp=ws, nbytes=big, lv=None):
        return (lib.oth_puct_begin, (env, None if p is None else ctypes.byref(p), wsp, nbytes,
                                     None if lv is None else ctypes.byref(lv), None))

    def advance(env, p, wsp=ws, nbytes=big, priors=arr, values=arr, lv=None):
        return (lib.oth_puct_advance, (env, None if p is None else ctypes.byref(p), wsp, nbytes, priors, values, 1,
                                       None if lv is None else ctypes.byref(lv), None))

    def result(env, p, wsp=ws, nbytes=big, v=arr):
        return (lib.oth_puct_result, (env, None if p is None else ctypes.byref(p), wsp, nbytes, v, None, None, None,
                                      None, None))

    cases = []
    for name, call in (("begin", begin), ("advance", advance), ("result", result)):
        cases += [
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
    for name, call in (("begin", begin), ("advance", advance)):
        cases += [
            (name + ": layout = 5", call(None, ok, lv=leaves(5, 0)), b"layout"),
            (name + ": layout = -1", call(None, ok, lv=leaves(-1, 0)), b"layout"),
            (name + ": dtype = 6", call(None, ok, lv=leaves(2, 6)), b"dtype"),
            # (a bad layout beside a NULL obs is not looked at: the call goes on to the NULL handle)
            (name + ": no obs", call(None, ok, lv=leaves(99, 99, obs=None)), b"oth_env"),
        ]
    cases += [
        ("advance: NULL priors", advance(None, ok, priors=None), b"priors"),
        ("advance: NULL values", advance(None, ok, values=None), b"values"),
        ("result: NULL visits", result(None, ok, v=None), b"visits"),
    ]

    def run():
        return [(what, fn(*args), lib.oth_last_error(), word) for what, (fn, args), word in cases]

    seen = on_a_thread(run)
    assert len(seen) == len(cases)
    for what, rc, msg, word in seen:
        assert rc == -1, what
        assert word in msg, (what, msg)
    assert list(out) == [0] * 64 and list(wsbuf) == [0] * 8  # nothing was written


def test_workspace_bytes(lib):
    def size(n, E, T):
        b = ctypes.c_uint64(0)
        rc = lib.oth_puct_workspace_bytes(n, E, T, ctypes.byref(b))
        return rc, b.value

    def run():
        bad = [(3, 4, 64), (17, 4, 4096), (8, 0, 4096), (8, 4, 63), (8, 4, (1 << 24) + 1), (16, 4, 255)]
        res = [(args, size(*args)[0], lib.oth_last_error()) for args in bad]
        res.append(("NULL bytes", lib.oth_puct_workspace_bytes(8, 4, 4096, None), lib.oth_last_error()))
        return res

    for what, rc, msg in on_a_thread(run):
        assert rc == -1 and msg, what
    for n in range(4, 17):
        W = (n * n + 63) // 64
        node = 3 * W + 4  # three boards of W words, w, v | P, the links, k | flags | square
        for E, T in ((1, n * n), (2, n * n + 1), (9, 4096), (70, 512), (65536, n * n), (7, 1 << 24)):
            rc, b = size(n, E, T)
            # a tag and a pad, two header words a board, the leaves in exchange format, the trees
            assert rc == 0 and b == 8 * (2 + 2 * E + 3 * W * E + (E + 3) // 4 + E * T * node), (n, E, T)
            assert b % 8 == 0
    assert size(8, 65536, 1 << 24)[1] >= 65536 * (1 << 24) * 16  # no 32-bit overflow
    # its own workspace: not the size of oth_mcts'
    m = ctypes.c_uint64(0)
    assert lib.oth_mcts_workspace_bytes(8, 4, 4096, ctypes.byref(m)) == 0 and m.value != size(8, 4, 4096)[1]


def test_python_surface():
    import torch

    import gymothelloenv_amd as g
    from gymothelloenv_amd import policies, vec_env
    assert g.PUCTPolicy is policies.PUCTPolicy and "PUCTPolicy" in policies.__all__
    for name in ("puct_quantize", "uniform_evaluator", "playout_evaluator", "PuctLeaves"):
        assert getattr(g, name) is getattr(vec_env, name)
    assert vec_env.PuctLeaves._fields == ("kind", "boards", "meta", "legal", "obs")
    pol = g.PUCTPolicy()
    assert (pol.simulations, pol.c, pol.counter) == (128, 1.25, 0)
    for name in ("reset", "get_action", "get_test_action", "seed"):
        assert callable(getattr(pol, name))
    pol.counter = 5
    pol.seed(9)
    assert pol.counter == 0
    with pytest.raises(ValueError, match="simulations"):
        g.PUCTPolicy(simulations=1)

    def defaults(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()][1:]

    V = vec_env.VecOthelloEnv
    assert defaults(V.puct_begin) == [("c", 1.25), ("max_tree_nodes", None), ("layout", "make_state"),
                                      ("dtype", torch.float32)]
    assert defaults(V.puct_advance) == [("priors", inspect.Parameter.empty), ("values", inspect.Parameter.empty),
                                        ("more", True)]
    assert defaults(V.puct_result) == [("value_sums", False), ("best", False), ("tree_nodes", False),
                                       ("status", False)]
    assert callable(V.puct_search) and callable(V.puct_actions)
    ev = g.playout_evaluator(3, seed=4)
    assert (ev.n_playouts, ev.seed, ev.counter) == (3, 4, 0)


def test_quantizer_on_the_host():
    """puct_quantize is torch alone: the masked softmax and both roundings, here on CPU tensors."""
    import torch

    from gymothelloenv_amd import puct_quantize
    logits = torch.tensor([[0.0, 1.0, 2.0, 3.0] * 4, [5.0] * 16, [0.0] * 16])
    legal = torch.tensor([[0b1010], [0xffff], [0]], dtype=torch.int64)
    priors, values = puct_quantize(logits, legal, torch.tensor([1.0, -1.0, 0.5]))
    assert priors.dtype == torch.int32 and values.tolist() == [32768, -32768, 16384]
    e = torch.exp(torch.tensor(2.0))
    want = [0, int(torch.round(65535 / (1 + e))), 0, int(torch.round(65535 * e / (1 + e)))]
    assert priors[0].tolist() == want + [0] * 12
    assert priors[1].tolist() == [4096] * 16 and not priors[2].any()
