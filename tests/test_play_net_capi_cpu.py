"""oth_play_net, oth_reset_vs_net and oth_step_vs_net without a GPU: every
argument check (each comes before the handle's device is touched, with nothing
launched -- the handle here is host memory that only says its board size), the
struct's layout and the Python surface."""
import ctypes
import inspect
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import net_cases as nc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


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


def handle(n=8, E=4):
    """Host memory with struct oth_env's first two fields (E, n) and zeros behind them: what the checks read."""
    buf = (ctypes.c_int32 * 128)()
    buf[0], buf[1] = E, n
    return buf


def policy(L=2, H=128, shifts=(5, 9), policy_shift=8, value_shift=3, blob=0x1000, blob_bytes=1 << 40, sample_discs=0):
    from gymothelloenv_amd import _lib as L_
    sh = list(shifts) + [0] * (4 - len(shifts))
    p = L_.OthNetParams(L, H, (ctypes.c_int32 * 4)(*sh), policy_shift, value_shift)
    return L_.OthNetPolicy(p, blob, blob_bytes, sample_discs)


BAD = [("layers = 0", dict(L=0), b"layers"), ("layers = 5", dict(L=5, shifts=(0,) * 4), b"layers"),
       ("width = 32", dict(H=32), b"width"), ("width = 96", dict(H=96), b"width"), ("width = 576", dict(H=576), b"width"),
       ("shift = 25", dict(shifts=(5, 25)), b"shift"), ("shift = -1", dict(shifts=(-1, 9)), b"shift"),
       ("policy_shift = 25", dict(policy_shift=25), b"policy_shift"), ("policy_shift = -1", dict(policy_shift=-1), b"policy_shift"),
       ("value_shift = 25", dict(value_shift=25), b"value_shift"), ("value_shift = -1", dict(value_shift=-1), b"value_shift"),
       ("NULL blob", dict(blob=None), b"blob"), ("misaligned blob", dict(blob=0x1008), b"aligned"),
       ("short blob", dict(blob_bytes=nc.blob_bytes(8, 2, 128) - 1), b"blob_bytes"),
       ("sample_discs = -1", dict(sample_discs=-1), b"sample_discs"),
       ("sample_discs = 258", dict(sample_discs=258), b"sample_discs")]


def test_struct_and_signatures(lib):
    from gymothelloenv_amd import _lib as L
    P, I32 = ctypes.c_void_p, ctypes.c_int32
    assert L.SIGNATURES["oth_play_net"] == (I32, [P, P, P, I32, P, P, P, P])
    assert L.SIGNATURES["oth_reset_vs_net"] == (I32, [P, P, P, P, P])
    assert L.SIGNATURES["oth_step_vs_net"] == (I32, [P, P, P, P, P, P, P, P])
    S = L.OthNetPolicy
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [("params", 0), ("blob", 32), ("blob_bytes", 40),
                                                                   ("sample_discs", 48)] and ctypes.sizeof(S) == 56
    assert L.OTH_NET_SAMPLE_DISCS_MAX == 257
    header = open(os.path.join(ROOT, "include", "othello_mi355x.h")).read()
    assert "#define OTH_NET_SAMPLE_DISCS_MAX 257" in header
    body = header[header.index("typedef struct oth_net_policy {"):header.index("} oth_net_policy;")]
    assert [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.splitlines()[1:] if ";" in ln] == \
        [f for f, _ in S._fields_]
    # exports == header, for the family's three calls (tests/test_capi_cpu.py holds the whole list)
    declared = set(re.findall(r"^int (oth_\w*_net)\(", header, re.M))
    assert declared == {"oth_play_net", "oth_reset_vs_net", "oth_step_vs_net"}
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()[-1].endswith("_net")}
    assert declared <= exported and {s for s in exported if s.startswith("oth_")} == declared
    for s in declared:
        assert getattr(lib, s) is not None
    assert "purpose 7" in header and "RNG_NET_MOVE = 7" in open(
        os.path.join(ROOT, "gymothelloenv_amd", "csrc", "state.hpp")).read()


def test_argument_checks_without_gpu(lib):
    h = handle()
    good = policy()
    out = (ctypes.c_int32 * 64)()
    arr = ctypes.cast(out, ctypes.c_void_p)

    def ref(p):
        return None if p is None else ctypes.addressof(p)

    def play(env=h, b=good, w=good, n_plies=2):
        return lib.oth_play_net, (env, ref(b), ref(w), n_plies, arr, arr, arr, None)

    def reset(env=h, o=good):
        return lib.oth_reset_vs_net, (env, ref(o), None, None, None)

    def step(env=h, o=good, actions=arr):
        return lib.oth_step_vs_net, (env, ref(o), actions, None, arr, arr, arr, None)

    keep = []
    cases = []
    for what, kw, word in BAD:
        bad = policy(**kw)
        keep.append(bad)
        cases += [("play, black: " + what, play(b=bad), word), ("play, white: " + what, play(w=bad), word),
                  ("reset_vs: " + what, reset(o=bad), word), ("step_vs: " + what, step(o=bad), word)]
    wide = policy(H=256, shifts=(5, 10))
    cases += [("play: NULL handle", play(env=None), b"oth_env"), ("reset_vs: NULL handle", reset(env=None), b"oth_env"),
              ("step_vs: NULL handle", step(env=None), b"oth_env"),
              ("play: NULL black", play(b=None), b"NULL"), ("play: NULL white", play(w=None), b"NULL"),
              ("reset_vs: NULL opponent", reset(o=None), b"NULL"), ("step_vs: NULL opponent", step(o=None), b"NULL"),
              ("play: n_plies = 0", play(n_plies=0), b"n_plies"), ("play: n_plies = -3", play(n_plies=-3), b"n_plies"),
              ("step_vs: NULL actions", step(actions=None), b"actions"),
              ("play: widths 128 and 256", play(w=wide), b"same width"),
              ("play: widths 256 and 128", play(b=wide), b"same width")]
    for n in (3, 17):  # a handle of a board size the network has no geometry for
        hn = handle(n=n)
        keep.append(hn)
        cases += [("play: board_size %d" % n, play(env=hn), b"board_size"),
                  ("reset_vs: board_size %d" % n, reset(env=hn), b"board_size"),
                  ("step_vs: board_size %d" % n, step(env=hn), b"board_size")]
    h16 = handle(n=16)  # what fits an 8 x 8 board is short for 16 x 16
    fits8 = policy(blob_bytes=nc.blob_bytes(8, 2, 128))
    cases += [("play: 8 x 8 bytes on 16 x 16", play(env=h16, b=fits8, w=fits8), b"blob_bytes")]

    def run():
        return [(what, fn(*args), lib.oth_last_error(), word) for what, (fn, args), word in cases]

    before = bytes(h), bytes(h16)
    seen = on_a_thread(run)
    assert len(seen) == len(cases) == 4 * len(BAD) + 12 + 6 + 1
    for what, rc, msg, word in seen:
        assert rc == -1, what
        assert msg and word in msg, (what, msg)
    assert list(out) == [0] * 64 and (bytes(h), bytes(h16)) == before  # nothing written, no ply counter moved


def test_python_surface():
    import gymothelloenv_amd as g
    from gymothelloenv_amd import net, policies, vec_env

    assert g.NetPlayer is net.NetPlayer and g.NetPolicy is policies.NetPolicy
    assert list(inspect.signature(net.NetPlayer.__init__).parameters)[1:] == ["net", "sample_discs"]
    assert list(inspect.signature(vec_env.VecOthelloEnv.play_net).parameters)[1:] == ["black", "white", "n_plies", "record"]
    assert list(inspect.signature(policies.NetPolicy.__init__).parameters)[1:3] == ["net", "sample_discs"]
    assert "NetPolicy" in policies.__all__
    with pytest.raises(TypeError):
        net.NetPlayer(object())
    with pytest.raises(TypeError):
        policies.NetPolicy("greedy")
