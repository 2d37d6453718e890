"""oth_play_cnet, oth_reset_vs_cnet and oth_step_vs_cnet without a GPU: every
argument check (each comes before the handle's device is touched, with nothing
launched -- the handle here is host memory that only says its board size), the
struct's layout and the Python surface."""
import ctypes
import inspect
import os
import re
import subprocess
import threading
import types

import pytest

import cnet_cases as cc

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


def policy(C=64, B=2, shift_stem=1, shifts=(9, 9, 10, 10), shift_head=9, policy_shift=8, value_shift=3, blob=0x1000,
           blob_bytes=1 << 40, sample_discs=0):
    from gymothelloenv_amd import _lib as L_
    sh = list(shifts) + [0] * (16 - len(shifts))
    p = L_.OthCnetParams(C, B, shift_stem, (ctypes.c_int32 * 16)(*sh), shift_head, policy_shift, value_shift)
    return L_.OthCnetPolicy(p, blob, blob_bytes, sample_discs)


BAD = [("channels = 32", dict(C=32), b"channels"), ("channels = 96", dict(C=96), b"channels"),
       ("channels = 256", dict(C=256), b"channels"), ("blocks = 0", dict(B=0), b"blocks"),
       ("blocks = 9", dict(B=9, shifts=(0,) * 16), b"blocks"),
       ("shift_stem = 25", dict(shift_stem=25), b"shift_stem"), ("shift_stem = -1", dict(shift_stem=-1), b"shift_stem"),
       ("shift = 25", dict(shifts=(9, 9, 10, 25)), b"shift"), ("shift = -1", dict(shifts=(-1, 9, 10, 10)), b"shift"),
       ("shift_head = 25", dict(shift_head=25), b"shift_head"), ("shift_head = -1", dict(shift_head=-1), b"shift_head"),
       ("policy_shift = 25", dict(policy_shift=25), b"policy_shift"), ("policy_shift = -1", dict(policy_shift=-1), b"policy_shift"),
       ("value_shift = 25", dict(value_shift=25), b"value_shift"), ("value_shift = -1", dict(value_shift=-1), b"value_shift"),
       ("NULL blob", dict(blob=None), b"blob"), ("misaligned blob", dict(blob=0x1008), b"aligned"),
       ("short blob", dict(blob_bytes=cc.blob_bytes(8, 2, 64) - 1), b"blob_bytes"),
       ("sample_discs = -1", dict(sample_discs=-1), b"sample_discs"),
       ("sample_discs = 258", dict(sample_discs=258), b"sample_discs")]


def test_struct_and_signatures(lib):
    from gymothelloenv_amd import _lib as L
    P, I32 = ctypes.c_void_p, ctypes.c_int32
    assert L.SIGNATURES["oth_play_cnet"] == L.SIGNATURES["oth_play_net"] == (I32, [P, P, P, I32, P, P, P, P])
    assert L.SIGNATURES["oth_reset_vs_cnet"] == L.SIGNATURES["oth_reset_vs_net"] == (I32, [P, P, P, P, P])
    assert L.SIGNATURES["oth_step_vs_cnet"] == L.SIGNATURES["oth_step_vs_net"] == (I32, [P, P, P, P, P, P, P, P])
    S = L.OthCnetPolicy
    assert ctypes.sizeof(L.OthCnetParams) == 88
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [("params", 0), ("blob", 88), ("blob_bytes", 96),
                                                                   ("sample_discs", 104)] and ctypes.sizeof(S) == 112
    header = open(os.path.join(ROOT, "include", "othello_mi355x.h")).read()
    body = header[header.index("typedef struct oth_cnet_policy {"):header.index("} oth_cnet_policy;")]
    fields = [ln.split(";")[0].split() for ln in body.splitlines()[1:] if ";" in ln]
    assert [f[-1].lstrip("*") for f in fields] == [f for f, _ in S._fields_]
    assert [" ".join(f[:-1]) + ("*" if f[-1].startswith("*") else "") for f in fields] == \
        ["oth_cnet_params", "const void*", "uint64_t", "int32_t"]
    # exports == header, for the family's three calls (tests/test_capi_cpu.py holds the whole list)
    declared = set(re.findall(r"^int (oth_(?:play|reset_vs|step_vs)_cnet)\(", header, re.M))
    assert declared == {"oth_play_cnet", "oth_reset_vs_cnet", "oth_step_vs_cnet"}
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines()}
    assert declared <= exported
    for s in declared:
        assert getattr(lib, s) is not None
    # the argument lists are the _net twins' but for the policy's type
    for s in declared:
        twin = s.replace("_cnet", "_net")
        a, b = (re.search(r"^int %s\((.*?)\);" % x, header, re.M | re.S).group(1) for x in (s, twin))
        assert " ".join(a.replace("oth_cnet_policy", "oth_net_policy").split()) == " ".join(b.split())


def test_argument_checks_without_gpu(lib):
    h = handle()
    good = policy()
    out = (ctypes.c_int32 * 64)()
    arr = ctypes.cast(out, ctypes.c_void_p)

    def ref(p):
        return None if p is None else ctypes.addressof(p)

    def play(env=h, b=good, w=good, n_plies=2):
        return lib.oth_play_cnet, (env, ref(b), ref(w), n_plies, arr, arr, arr, None)

    def reset(env=h, o=good):
        return lib.oth_reset_vs_cnet, (env, ref(o), None, None, None)

    def step(env=h, o=good, actions=arr):
        return lib.oth_step_vs_cnet, (env, ref(o), actions, None, arr, arr, arr, None)

    keep = []
    cases = []
    for what, kw, word in BAD:
        bad = policy(**kw)
        keep.append(bad)
        cases += [("play, black: " + what, play(b=bad), word), ("play, white: " + what, play(w=bad), word),
                  ("reset_vs: " + what, reset(o=bad), word), ("step_vs: " + what, step(o=bad), word)]
    wide = policy(C=128)
    cases += [("play: NULL handle", play(env=None), b"oth_env"), ("reset_vs: NULL handle", reset(env=None), b"oth_env"),
              ("step_vs: NULL handle", step(env=None), b"oth_env"),
              ("play: NULL black", play(b=None), b"NULL"), ("play: NULL white", play(w=None), b"NULL"),
              ("reset_vs: NULL opponent", reset(o=None), b"NULL"), ("step_vs: NULL opponent", step(o=None), b"NULL"),
              ("play: n_plies = 0", play(n_plies=0), b"n_plies"), ("play: n_plies = -3", play(n_plies=-3), b"n_plies"),
              ("step_vs: NULL actions", step(actions=None), b"actions"),
              ("play: channels 64 and 128", play(w=wide), b"same channels"),
              ("play: channels 128 and 64", play(b=wide), b"same channels")]
    for n in (3, 17):  # a handle of a board size the network has no geometry for
        hn = handle(n=n)
        keep.append(hn)
        cases += [("play: board_size %d" % n, play(env=hn), b"board_size"),
                  ("reset_vs: board_size %d" % n, reset(env=hn), b"board_size"),
                  ("step_vs: board_size %d" % n, step(env=hn), b"board_size")]
    h16 = handle(n=16)  # what fits an 8 x 8 board is short for 16 x 16
    fits8 = policy(blob_bytes=cc.blob_bytes(8, 2, 64))
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


def fake_net(cls, n, device="cuda:0", **attrs):
    """A network object without a device: what NetPlayer reads of it."""
    import torch
    from gymothelloenv_amd import _lib as L
    net = cls.__new__(cls)
    net.board_size, net.device = n, torch.device(device)
    net.blob = torch.zeros(64, dtype=torch.uint8)
    net.params = L.OthCnetParams() if "channels" in attrs else L.OthNetParams()
    for k, v in attrs.items():
        setattr(net, k, v)
    return net


def test_python_surface():
    import torch
    import gymothelloenv_amd as g
    from gymothelloenv_amd import _lib as L
    from gymothelloenv_amd import cnet, net, policies, vec_env

    assert list(inspect.signature(net.NetPlayer.__init__).parameters)[1:] == ["net", "sample_discs"]
    conv64 = fake_net(cnet.DeviceConvNet, 8, channels=64, blocks=3)
    conv128 = fake_net(cnet.DeviceConvNet, 8, channels=128, blocks=1)
    mlp = fake_net(net.DeviceNet, 8, layers=2, width=128)
    a, b, m = g.NetPlayer(conv64, 12), g.NetPlayer(conv128), g.NetPlayer(mlp)
    assert (a.kind, b.kind, m.kind) == ("conv", "conv", "mlp")
    assert isinstance(a._struct, L.OthCnetPolicy) and isinstance(m._struct, L.OthNetPolicy)
    assert a._struct.blob == conv64.blob.data_ptr() and a._struct.blob_bytes == 64 and a._struct.sample_discs == 12
    assert a.net is conv64  # the player keeps the blob alive
    assert repr(a) == "NetPlayer(<8 x 8, conv, 3 blocks of 64 channels>, sample_discs=12)"
    assert repr(m) == "NetPlayer(<8 x 8, 2 layers of 128>, sample_discs=0)"
    with pytest.raises(TypeError):
        net.NetPlayer(object())
    for bad in (-1, 258, 1.5, True):
        with pytest.raises(ValueError):
            net.NetPlayer(conv64, bad)
    assert isinstance(policies.NetPolicy(conv64, 5).player._struct, L.OthCnetPolicy)
    # the env's dispatch: errors raised before any call (the env here has no handle to call with)
    env = types.SimpleNamespace(board_size=8, device=torch.device("cuda:0"), num_envs=4)
    play = vec_env.VecOthelloEnv.play_net
    with pytest.raises(ValueError, match="one kind"):
        play(env, a, m)
    with pytest.raises(ValueError, match="one kind"):
        play(env, m, a)
    with pytest.raises(ValueError, match="same channels"):
        play(env, a, b)
    with pytest.raises(TypeError):
        play(env, a, "greedy")
    with pytest.raises(ValueError, match="6 x 6"):
        play(types.SimpleNamespace(board_size=6, device=torch.device("cuda:0"), num_envs=4), a)
    with pytest.raises(ValueError, match="lives on"):
        play(types.SimpleNamespace(board_size=8, device=torch.device("cuda:1"), num_envs=4), a)
    with pytest.raises(ValueError, match="6 x 6"):
        a._policy(types.SimpleNamespace(board_size=6, device=torch.device("cuda:0")))
