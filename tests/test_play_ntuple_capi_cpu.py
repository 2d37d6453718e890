"""oth_play_ntuple, oth_reset_vs_ntuple, oth_step_vs_ntuple and oth_ntuple_update_masked
without a GPU: every argument check (each comes before the handle's device is touched,
with nothing launched -- the handle here is host memory that only says its board size),
the masked update's refusals, the exports and the Python surface."""
import ctypes
import inspect
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import ntuple_cases as nc
import ntuple_ref as nr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TUPLES = nc.tuples(8, 5, "mixed")
COUNT = nr.weight_count(TUPLES)
PLAN_BYTES = 4 * (8 + 18 * len(TUPLES))


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


def params(tp=TUPLES, shift=3, **fields):
    from gymothelloenv_amd import _lib as L
    p = nc.fill_params(L.OthNtupleParams(), tp, shift)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def policy(p=None, plan=0x1000, plan_bytes=1 << 20, weights=0x2000, weight_count=COUNT, depth=2, terminal=64,
           endgame=0, explore=0, max_nodes=100):
    from gymothelloenv_amd import _lib as L
    return L.OthNtuplePolicy(params() if p is None else p, plan, plan_bytes, weights, weight_count, depth, terminal,
                             endgame, explore, max_nodes)


def bad_policies():
    """(what, policy, a word of the message)"""
    out = [("tuples = 0", policy(params(tuples=0)), b"tuples"), ("tuples = 33", policy(params(tuples=33)), b"tuples"),
           ("value_shift = -1", policy(params(value_shift=-1)), b"value_shift"),
           ("value_shift = 25", policy(params(value_shift=25)), b"value_shift")]
    p = params()
    p.length[4] = 9
    out.append(("length = 9", policy(p), b"length"))
    p = params()
    p.squares[2][1] = 64
    out.append(("square = 64", policy(p), b"squares"))
    p = params()
    p.squares[0][7] = p.squares[0][2]
    out.append(("a square twice", policy(p), b"distinct"))
    out += [("NULL plan", policy(plan=None), b"plan"), ("misaligned plan", policy(plan=0x1004), b"aligned"),
            ("short plan", policy(plan_bytes=PLAN_BYTES - 1), b"plan_bytes"),
            ("NULL weights", policy(weights=None), b"weights"),
            ("short weights", policy(weight_count=COUNT - 1), b"weight_count"),
            ("depth = 0", policy(depth=0), b"depth"), ("depth = 15", policy(depth=15), b"depth"),
            ("terminal = 0", policy(terminal=0), b"terminal_weight"),
            ("terminal = 32768", policy(terminal=32768), b"terminal_weight"),
            ("endgame_empties = -1", policy(endgame=-1), b"endgame_empties"),
            ("endgame_empties = 15", policy(endgame=15), b"endgame_empties"),
            ("explore = -1", policy(explore=-1), b"explore"), ("explore = 65537", policy(explore=65537), b"explore"),
            ("max_nodes = 0", policy(max_nodes=0), b"max_nodes"), ("max_nodes = 2^32", policy(max_nodes=1 << 32), b"max_nodes")]
    return out


def test_struct_signatures_and_exports(lib):
    from gymothelloenv_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "othello_mi355x.h")).read()
    declared = set(re.findall(r"^int (oth_(?:play|reset_vs|step_vs)_ntuple|oth_ntuple_update_masked)\(", header, re.M))
    assert declared == {"oth_play_ntuple", "oth_reset_vs_ntuple", "oth_step_vs_ntuple", "oth_ntuple_update_masked"}
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines()}
    assert declared <= exported
    for s in declared:
        assert s in L.SIGNATURES and getattr(lib, s) is not None
    # the good policy of this file really is good up to the launch: the exploring bounds are inclusive
    assert ctypes.sizeof(L.OthNtuplePolicy) == ctypes.sizeof(L.OthNtupleParams) + 56


def test_argument_checks_without_gpu(lib):
    from gymothelloenv_amd import _lib as L
    h = handle()
    good = policy()
    out = (ctypes.c_int64 * 64)()
    arr = ctypes.cast(out, ctypes.c_void_p)

    def ref(p):
        return None if p is None else ctypes.addressof(p)

    def td(**null):
        f = dict(boards=arr.value, meta=arr.value, targets=arr.value, learn=arr.value)
        f.update(null)
        return L.OthNtupleTd(f["boards"], f["meta"], f["targets"], f["learn"])

    def play(env=h, b=good, w=good, n_plies=2, rows=None):
        return lib.oth_play_ntuple, (env, ref(b), ref(w), n_plies, arr, arr, arr, arr, ref(rows), None)

    def reset(env=h, o=good):
        return lib.oth_reset_vs_ntuple, (env, ref(o), None, None, None)

    def step(env=h, o=good, actions=arr):
        return lib.oth_step_vs_ntuple, (env, ref(o), actions, None, arr, arr, arr, arr, None)

    keep, cases = [], []
    bad = bad_policies()
    for what, p, word in bad:
        keep.append(p)
        cases += [("play, black: " + what, play(b=p), word), ("play, white: " + what, play(w=p), word),
                  ("reset_vs: " + what, reset(o=p), word), ("step_vs: " + what, step(o=p), word)]
    cases += [("play: NULL handle", play(env=None), b"oth_env"), ("reset_vs: NULL handle", reset(env=None), b"oth_env"),
              ("step_vs: NULL handle", step(env=None), b"oth_env"),
              ("play: NULL black", play(b=None), b"NULL"), ("play: NULL white", play(w=None), b"NULL"),
              ("reset_vs: NULL opponent", reset(o=None), b"NULL"), ("step_vs: NULL opponent", step(o=None), b"NULL"),
              ("play: n_plies = 0", play(n_plies=0), b"n_plies"), ("play: n_plies = -3", play(n_plies=-3), b"n_plies"),
              ("step_vs: NULL actions", step(actions=None), b"actions")]
    for member in ("boards", "meta", "targets", "learn"):
        rows = td(**{member: None})
        keep.append(rows)
        cases.append(("play: td with NULL %s" % member, play(rows=rows), b"td"))
    for n in (3, 17):  # a handle of a board size the network has no geometry for
        hn = handle(n=n)
        keep.append(hn)
        cases += [("play: board_size %d" % n, play(env=hn), b"board_size"),
                  ("reset_vs: board_size %d" % n, reset(env=hn), b"board_size"),
                  ("step_vs: board_size %d" % n, step(env=hn), b"board_size")]
    h4 = handle(n=4)  # a square of an 8 x 8 board is out of range on 4 x 4
    cases.append(("play: 8 x 8 tuples on 4 x 4", play(env=h4), b"squares"))

    def run():
        return [(what, fn(*args), lib.oth_last_error(), word) for what, (fn, args), word in cases]

    before = bytes(h), bytes(h4)
    seen = on_a_thread(run)
    assert len(seen) == len(cases) == 4 * len(bad) + 10 + 4 + 6 + 1
    for what, rc, msg, word in seen:
        assert rc == -1, what
        assert msg and word in msg, (what, msg)
    assert list(out) == [0] * 64 and (bytes(h), bytes(h4)) == before  # nothing written, no ply counter moved


def test_masked_update_refusals_without_gpu(lib):
    out = (ctypes.c_int64 * 64)()
    arr = ctypes.cast(out, ctypes.c_void_p)
    plan = np.zeros(512, dtype=np.uint64)
    good = params()

    def up(n=8, R=4, p=good, plan_=plan.ctypes.data, nbytes=1 << 20, w=arr, wc=COUNT, boards=arr, meta=arr, targets=arr,
           mask=arr, rate=1, rate_shift=0, deltas=arr):
        return (n, R, None if p is None else ctypes.byref(p), plan_, nbytes, w, wc, boards, meta, targets, mask, rate,
                rate_shift, deltas, None)

    cases = [("tuples = 0", up(p=params(tuples=0)), b"tuples"), ("NULL params", up(p=None), b"params"),
             ("NULL plan", up(plan_=None), b"plan"), ("misaligned plan", up(plan_=plan.ctypes.data + 4), b"aligned"),
             ("short plan", up(nbytes=PLAN_BYTES - 1), b"plan_bytes"), ("NULL weights", up(w=None), b"weights"),
             ("short weights", up(wc=COUNT - 1), b"weight_count"), ("board_size = 3", up(n=3), b"board_size"),
             ("board_size = 17", up(n=17), b"board_size"), ("NULL boards", up(boards=None), b"boards"),
             ("NULL meta", up(meta=None), b"meta"), ("NULL targets", up(targets=None), b"targets"),
             ("NULL deltas", up(deltas=None), b"deltas"), ("n_rows = -1", up(R=-1), b"n_rows"),
             ("n_rows = 2^24 + 1", up(R=(1 << 24) + 1), b"n_rows"), ("rate = -1", up(rate=-1), b"rate"),
             ("rate = 2^24 + 1", up(rate=(1 << 24) + 1), b"rate"), ("rate_shift = -1", up(rate_shift=-1), b"rate_shift"),
             ("rate_shift = 41", up(rate_shift=41), b"rate_shift")]
    for mask in (arr, None):  # with a mask and without one
        def run():
            res = []
            for what, args, word in cases:
                a = list(args)
                a[10] = a[10] if mask is not None else None
                res.append((what, lib.oth_ntuple_update_masked(*a), lib.oth_last_error(), word))
            return res
        for what, rc, msg, word in on_a_thread(run):
            assert rc == -1, what
            assert msg and word in msg, (what, msg)
    assert list(out) == [0] * 64 and not plan.any()
    assert lib.oth_ntuple_update_masked(*up(R=0)) == 0  # no rows: nothing to launch


def test_python_surface():
    import gymothelloenv_amd as g
    from gymothelloenv_amd import ntuple, policies, vec_env

    assert g.NTuplePlayer is ntuple.NTuplePlayer is policies.NTuplePlayer and g.TDRows is ntuple.TDRows
    assert list(inspect.signature(ntuple.NTuplePlayer.__init__).parameters)[1:] == [
        "net", "depth", "endgame_empties", "explore", "terminal", "max_nodes"]
    assert list(inspect.signature(vec_env.VecOthelloEnv.play_ntuple).parameters)[1:] == [
        "black", "white", "n_plies", "record", "fallbacks", "td"]
    assert list(inspect.signature(ntuple.NTupleNet.update).parameters)[1:] == [
        "boards", "meta", "targets", "rate", "rate_shift", "mask"]
    assert list(inspect.signature(ntuple.NTupleNet.td_play).parameters)[1:] == [
        "env", "n_plies", "rate", "rate_shift", "explore", "depth"]
    assert ntuple.TDRows._fields == ("boards", "meta", "targets", "learn")
    with pytest.raises(TypeError):
        ntuple.NTuplePlayer(object())
