"""The replay store's C ABI without a GPU: oth_replay_workspace_bytes, which needs
no handle, every argument check that comes before a handle is needed (with
nothing launched), and the Python surface."""
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


def words(n, E, H, B):
    """The layout of csrc/replay.hpp, restated: tags, headers, state bytes, outcomes, a count word a chunk, the
    prefix, the staging rows, the rows' discs and visits."""
    W, R, C = (n * n + 63) // 64, E * H, (E * H + 1023) // 1024
    return (2 + 2 * E + (R + 7) // 8 + (R + 1) // 2 + C + (C + 2) // 2 + (B + 3) // 4 + 3 * W * B + 3 * W * R +
            (R * n * n + 1) // 2)


def test_workspace_bytes(lib):
    from gymothelloenv_amd import _lib as L
    assert (L.OTH_REPLAY_MAX_HORIZON, L.OTH_REPLAY_MAX_ROWS, L.OTH_REPLAY_MAX_BATCH) == (65536, 1 << 24, 1 << 20)
    assert (L.OTH_REPLAY_EMPTY, L.OTH_REPLAY_OPEN, L.OTH_REPLAY_LABELLED) == (0, 1, 2)

    def size(n, E, H, B):
        b = ctypes.c_uint64(0)
        return lib.oth_replay_workspace_bytes(n, E, H, B, ctypes.byref(b)), b.value

    def run():
        bad = [(3, 4, 8, 8), (17, 4, 8, 8), (8, 0, 8, 8), (8, -1, 8, 8), (8, 4, 0, 8), (8, 4, 65537, 8), (8, 4, 8, 0),
               (8, 4, 8, (1 << 20) + 1), (8, 257, 65536, 8), (8, (1 << 24) + 1, 1, 8), (8, 1 << 30, 1 << 16, 8)]
        res = [(args, size(*args), lib.oth_last_error()) for args in bad]
        res.append(("NULL bytes", (lib.oth_replay_workspace_bytes(8, 4, 8, 8, None), 0), lib.oth_last_error()))
        return res

    for what, (rc, b), msg in on_a_thread(run):
        assert rc == -1 and msg and b == 0, what
    for n in (4, 6, 8, 9, 12, 16):
        for E, B in ((1, 1), (5, 19), (37, 4096), (256, 1 << 20)):
            last = 0
            for H in (1, 3, 31, 1024, 65536):
                if E * H > 1 << 24:
                    continue
                rc, b = size(n, E, H, B)
                assert rc == 0 and b == 8 * words(n, E, H, B), (n, E, H, B)
                assert b > last, "the size grows with the horizon"
                last = b
            if B + 4 <= 1 << 20:
                assert size(n, E, 3, B + 1)[1] >= size(n, E, 3, B)[1] and size(n, E, 3, B + 4)[1] > size(n, E, 3, B)[1]
            assert size(n, E + 1, 3, B)[1] > size(n, E, 3, B)[1]
    assert size(8, 256, 65536, 1 << 20) == (0, 8 * words(8, 256, 65536, 1 << 20))  # the largest store


def test_argument_checks_without_gpu(lib):
    from gymothelloenv_amd import _lib as L
    out = (ctypes.c_int32 * 64)()
    arr = ctypes.cast(out, ctypes.c_void_p)
    wsbuf = (ctypes.c_uint64 * 8)()
    ws = ctypes.cast(wsbuf, ctypes.c_void_p)
    # the stand-in of tests/test_puct_capi_cpu.py: a block that holds only n_envs = 4, board_size = 8, W = 1
    blank = ctypes.create_string_buffer(struct.pack("<iii", 4, 8, 1), 512)
    h = ctypes.cast(blank, ctypes.c_void_p)
    wide = ctypes.cast(ctypes.create_string_buffer(struct.pack("<iii", 1 << 20, 8, 1), 512), ctypes.c_void_p)
    big = 1 << 50
    need = ctypes.c_uint64(0)
    assert lib.oth_replay_workspace_bytes(8, 4, 8, 16, ctypes.byref(need)) == 0

    def batch(layout=2, dtype=3, obs=arr):
        return L.OthReplayBatch(None, None, None, None, None, None, obs, layout, dtype, None, None)

    def ref(x):
        return None if x is None else ctypes.byref(x)

    plain = batch(obs=None)

    def begin(env, H=8, B=16, wsp=ws, nbytes=big, **kw):
        return lib.oth_replay_begin, (env, H, B, wsp, nbytes, None)

    def append(env, H=8, B=16, wsp=ws, nbytes=big, visits=arr, **kw):
        return lib.oth_replay_append, (env, H, B, wsp, nbytes, visits, None, None)

    def label(env, H=8, B=16, wsp=ws, nbytes=big, rewards=arr, dones=arr, **kw):
        return lib.oth_replay_label, (env, H, B, wsp, nbytes, rewards, dones, None)

    def counts(env, H=8, B=16, wsp=ws, nbytes=big, outp=arr, **kw):
        return lib.oth_replay_counts, (env, H, B, wsp, nbytes, outp, None)

    def gather(env, H=8, B=16, wsp=ws, nbytes=big, n=4, rows=arr, b=plain, **kw):
        return lib.oth_replay_gather, (env, H, B, wsp, nbytes, n, rows, None, ref(b), None)

    def sample(env, H=8, B=16, wsp=ws, nbytes=big, n=4, b=plain, **kw):
        return lib.oth_replay_sample, (env, H, B, wsp, nbytes, n, 1, 0, 0, 0, ref(b), None)

    cases = []
    for name, call in (("begin", begin), ("append", append), ("label", label), ("counts", counts), ("gather", gather),
                       ("sample", sample)):
        cases += [
            (name + ": NULL workspace", call(None, wsp=None), b"workspace"),
            (name + ": horizon = 0", call(None, H=0), b"horizon"),
            (name + ": horizon = 65537", call(h, H=65537), b"horizon"),
            (name + ": max_batch = 0", call(None, B=0), b"max_batch"),
            (name + ": max_batch = 2^20 + 1", call(h, B=(1 << 20) + 1), b"max_batch"),
            (name + ": misaligned workspace", call(None, wsp=ctypes.c_void_p(ws.value + 4)), b"aligned"),
            (name + ": NULL handle", call(None), b"oth_env"),
            (name + ": n_envs * horizon above 2^24", call(wide, H=17), b"n_envs * horizon"),
            (name + ": workspace_bytes too small", call(h, nbytes=need.value - 1), b"workspace_bytes"),
        ]
    for name, call in (("gather", gather), ("sample", sample)):
        cases += [
            (name + ": NULL batch", call(None, b=None), b"batch"),
            (name + ": n = 0", call(None, n=0), b"n must"),
            (name + ": n = -3", call(h, n=-3), b"n must"),
            (name + ": n above max_batch", call(h, n=17), b"n must"),
            (name + ": layout = 5", call(None, b=batch(layout=5)), b"layout"),
            (name + ": layout = -1", call(None, b=batch(layout=-1)), b"layout"),
            (name + ": dtype = 6", call(None, b=batch(dtype=6)), b"dtype"),
            (name + ": no obs", call(None, b=batch(99, 99, obs=None)), b"oth_env"),
        ]
    cases += [
        ("append: NULL visits", append(None, visits=None), b"visits"),
        ("label: NULL rewards", label(None, rewards=None), b"rewards"),
        ("label: NULL dones", label(None, dones=None), b"dones"),
        ("counts: NULL out", counts(None, outp=None), b"out"),
        ("gather: NULL rows_in", gather(None, rows=None), b"rows_in"),
    ]
    other = ctypes.cast((ctypes.c_uint64 * 8)(), ctypes.c_void_p)
    for what, args in (("NULL sym", (8, 1, 1, None, arr, other, None)), ("NULL in", (8, 1, 1, arr, None, other, None)),
                       ("NULL out", (8, 1, 1, arr, arr, None, None)), ("in == out", (8, 1, 1, arr, other, other, None)),
                       ("n = 0", (8, 0, 1, arr, arr, other, None)), ("planes = 0", (8, 1, 0, arr, arr, other, None)),
                       ("n * planes above 2^31 - 1", (8, 1 << 30, 2, arr, arr, other, None)),
                       ("board_size = 3", (3, 1, 1, arr, arr, other, None)),
                       ("board_size = 17", (17, 1, 1, arr, arr, other, None))):
        cases.append(("symmetry_masks: " + what, (lib.oth_symmetry_masks, args), b""))

    def run():
        return [(what, fn(*args), lib.oth_last_error(), word) for what, (fn, args), word in cases]

    seen = on_a_thread(run)
    assert len(seen) == len(cases)
    for what, rc, msg, word in seen:
        assert rc == -1, what
        assert msg and word in msg, (what, msg)
    assert list(out) == [0] * 64 and list(wsbuf) == [0] * 8  # nothing was written


def test_python_surface():
    import torch

    import gymothelloenv_amd as g
    from gymothelloenv_amd import _lib as L
    from gymothelloenv_amd import vec_env

    def defaults(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()][1:]

    V = vec_env.VecOthelloEnv
    empty = inspect.Parameter.empty
    assert defaults(V.replay_begin) == [("horizon", empty), ("max_batch", 4096)]
    assert defaults(V.replay_append) == [("visits", empty), ("skip", None)]
    assert defaults(V.replay_label) == [("rewards", empty), ("dones", empty)]
    assert defaults(V.replay_counts) == []
    assert defaults(V.replay_gather)[:4] == [("rows", empty), ("sym", None), ("layout", "make_state"),
                                             ("dtype", torch.float32)]
    assert defaults(V.replay_sample)[:4] == [("n", empty), ("augment", True), ("seed", None), ("counter", None)]
    assert isinstance(V.replay_sample_counter, property)
    assert "record=True" in V.puct_play.__doc__  # a keyword beside begin_kw: the signature stays as it is
    assert g.ReplayBatch._fields == ("state", "boards", "meta", "legal", "visits", "outcome", "obs", "rows", "sym")
    assert g.symmetry_masks is vec_env.symmetry_masks
    # struct oth_replay_batch: nine pointers and two ints, in the header's order
    S = L.OthReplayBatch
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [
        ("state", 0), ("boards", 8), ("meta", 16), ("legal", 24), ("visits", 32), ("outcome", 40), ("obs", 48),
        ("layout", 56), ("dtype", 60), ("rows", 64), ("sym", 72)]
    import replay_ref as rr
    for n in range(4, 17):
        p = g.symmetry_permutations(n)
        assert p.dtype == torch.int64 and tuple(p.shape) == (8, n * n)
        assert (p.numpy() == rr.permutations(n)).all()
