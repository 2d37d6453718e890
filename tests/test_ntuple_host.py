"""The n-tuple network's core (csrc/ntuple.hpp: the plan, cell code, index, sum, value,
delta, the additions and the search's leaf rule -- the text the device kernels run,
compiled for the host with g++: tests/host/ntuple_host.cpp) against the numpy of
tests/ntuple_ref.py on every case of tests/ntuple_cases.py, with guard words behind
every output.  Every comparison is exact equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ntuple_cases as nc
import ntuple_ref as nr
import search_ref as sh

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "ntuple_host.cpp")
LIB = os.path.join(HERE, "host", "libntuple_host.so")
HDRS = [os.path.join(ROOT, "gymothelloenv_amd", "csrc", f) for f in ("ntuple.hpp", "search.hpp", "root_tasks.hpp",
                                                                      "bitboard.hpp")]
GUARD = 64  # elements behind an output that no call may touch


def load_hostlib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    P, I = ctypes.c_void_p, ctypes.c_int
    L.host_ntuple_weight_count.restype = ctypes.c_uint64
    L.host_ntuple_weight_count.argtypes = [I, P]
    L.host_ntuple_plan.restype = ctypes.c_uint64
    L.host_ntuple_plan.argtypes = [I, P, P, ctypes.c_uint64]
    L.host_ntuple_eval.argtypes = [I, I, P, P, P, P, P, P]
    L.host_ntuple_update.argtypes = [I, I, P, P, P, P, P, ctypes.c_int32, ctypes.c_int32, P]
    L.host_search_ntuple.argtypes = [I, I, P, P, P, I, P, P, I, ctypes.c_uint64, P, P, P, P, P]
    return L


@pytest.fixture(scope="module")
def hostlib():
    return load_hostlib()


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def guarded(count, dtype, fill=7):
    whole = np.full(count + GUARD, fill, dtype=dtype)
    return whole, whole[:count]


def host_eval(L, c, shift, R, sums=True):
    p = nc.params(c.tuples, shift)
    vw, values = guarded(R, np.int32)
    sw, sm = guarded(R, np.int64)
    w = c.weights.copy()
    assert L.host_ntuple_eval(c.n, R, ctypes.byref(p), ptr(w), ptr(c.boards), ptr(c.meta), ptr(values),
                              ptr(sm) if sums else None) == 0
    assert (vw[R:] == 7).all() and (sw[R:] == 7).all(), "the call wrote behind its output"
    assert (w == c.weights).all()
    return values.copy(), (sm.copy() if sums else None)


def host_update(L, c, shift, R, weights, rate, rate_shift, targets=None):
    p = nc.params(c.tuples, shift)
    count = nr.weight_count(c.tuples)
    ww, w = guarded(count, np.int32)
    w[:] = weights
    dw, d = guarded(R, np.int32)
    tg = np.ascontiguousarray(c.targets[:R] if targets is None else targets)
    assert L.host_ntuple_update(c.n, R, ctypes.byref(p), ptr(w), ptr(c.boards), ptr(c.meta), ptr(tg), rate, rate_shift,
                                ptr(d)) == 0
    assert (ww[count:] == 7).all() and (dw[R:] == 7).all(), "the call wrote behind its output"
    return w.copy(), d.copy()


def host_search(L, s, depth, tp, shift, weights, terminal=64, max_nodes=1 << 22):
    """The five outputs of the host build on State s."""
    nn, E = s.n * s.n, s.E
    p = nc.params(tp, shift)
    outs = [guarded(E, np.int32), guarded(E, np.int32), guarded(E * nn, np.int32), guarded(E, np.uint8),
            guarded(E, np.uint64)]
    w = np.ascontiguousarray(weights, dtype=np.int32)
    assert L.host_search_ntuple(s.n, E, ptr(s.boards), ptr(s.meta), ptr(s.legal), depth, ctypes.byref(p), ptr(w), terminal,
                                max_nodes, *[ptr(o[1]) for o in outs]) == 0
    for (whole, part) in outs:
        assert (whole[part.size:] == 7).all(), "the call wrote behind its output"
    got = [o[1].copy() for o in outs]
    got[2] = got[2].reshape(E, nn)
    return got


def test_params_layout():
    from gymothelloenv_amd import _lib as L
    for S in (L.OthNtupleParams, nc.Params):
        assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [("tuples", 0), ("length", 4), ("squares", 132),
                                                                       ("value_shift", 1156)]
        assert ctypes.sizeof(S) == 1160


def test_sigma_is_the_replay_symmetry():
    """ntuple_ref.sigma against the replay store's permutations (tests/replay_cases.py writes them from the header)."""
    for n in (4, 7, 16):
        seen = set()
        for s in range(8):
            perm = [nr.sigma(n, s, a) for a in range(n * n)]
            assert sorted(perm) == list(range(n * n))
            seen.add(tuple(perm))
        assert len(seen) == 8 and [nr.sigma(n, 0, a) for a in range(n * n)] == list(range(n * n))
        assert nr.sigma(n, 1, 1) == n and nr.sigma(n, 2, 0) == (n - 1) * n and nr.sigma(n, 4, 0) == n - 1


@pytest.mark.parametrize("cfg", nc.CONFIGS, ids=nc.CONFIG_IDS)
def test_eval_against_the_reference(hostlib, cfg):
    c = nc.case(*cfg)
    nc.check_rows(c)
    assert hostlib.host_ntuple_weight_count(c.n, ctypes.byref(nc.params(c.tuples, 0))) == nr.weight_count(c.tuples)
    for shift in nc.SHIFTS:
        want_v, want_s = nr.evaluate(c.n, c.tuples, shift, c.weights, c.boards, c.meta)
        clamped = np.abs(want_s >> shift) > 32768
        assert clamped.any() if shift == 0 else not clamped.any()
        for R in nc.ROWS:
            v, s = host_eval(hostlib, c, shift, R)
            np.testing.assert_array_equal(v, want_v[:R])
            np.testing.assert_array_equal(s, want_s[:R])
        np.testing.assert_array_equal(host_eval(hostlib, c, shift, 65, sums=False)[0], want_v[:65])


def test_rows_do_not_read_what_the_header_excludes(hostlib):
    """Other meta bits, bits at and above nn, and the opponent's bit under the mover's change nothing."""
    c = nc.case(6, 5, "mixed")
    nn, W = 36, 1
    v, s = host_eval(hostlib, c, 0, 257)
    clean = c._replace(meta=(c.meta & 1).astype(np.uint16), boards=c.boards & np.uint64((1 << nn) - 1))
    tw = (c.meta & 1) != 0
    b = clean.boards.copy()
    both = b[:, 0] & b[:, 1]
    b[:, 0] &= ~np.where(tw, both, np.uint64(0))  # the opponent's bit on a square set in both
    b[:, 1] &= ~np.where(tw, np.uint64(0), both)
    clean = clean._replace(boards=b)
    assert (clean.boards != c.boards).any()
    v2, s2 = host_eval(hostlib, clean, 0, 257)
    np.testing.assert_array_equal(v, v2)
    np.testing.assert_array_equal(s, s2)


@pytest.mark.parametrize("cfg", nc.CONFIGS, ids=nc.CONFIG_IDS)
def test_update_against_the_reference(hostlib, cfg):
    c = nc.case(*cfg)
    for shift, (name, rate, rate_shift) in zip((0, 9, 0, 9, 0), nc.RATES):
        for R in (nc.ROWS if name == "plain" else (257,)):
            sub = c._replace(boards=c.boards[:R], meta=c.meta[:R], targets=c.targets[:R])
            want_w, want_d = nr.update(c.n, c.tuples, shift, c.weights, sub.boards, sub.meta, sub.targets, rate, rate_shift)
            w, d = host_update(hostlib, sub, shift, R, c.weights, rate, rate_shift)
            np.testing.assert_array_equal(d, want_d, err_msg=name)
            np.testing.assert_array_equal(w, want_w, err_msg=name)
            if name == "zero":
                assert not d.any() and (w == c.weights).all()
            if name == "largest" and R:
                assert (np.abs(d.astype(np.int64)) == 1 << 30).any(), "no delta reached the clamp"


def test_update_special_cases(hostlib):
    # maximal contention: every row hits the same three entries eight times
    c = nc.case(4, 1, "ones")._replace(tuples=[[5]])
    c = c._replace(weights=np.array([100, -200, 300, 7], dtype=np.int32))
    want_w, want_d = nr.update(4, c.tuples, 0, c.weights, c.boards, c.meta, c.targets, 3000, 10)
    w, d = host_update(hostlib, c, 0, 257, c.weights, 3000, 10)
    np.testing.assert_array_equal(w, want_w)
    np.testing.assert_array_equal(d, want_d)
    assert (w != c.weights).all()
    # a weight that wraps: 2^31 - 5 plus positive deltas
    wrap = c.weights.copy()
    wrap[:] = 2 ** 31 - 5
    tg = np.full(257, 40000, dtype=np.int32)
    want_w, want_d = nr.update(4, c.tuples, 24, wrap, c.boards, c.meta, tg, 1, 0)
    assert (want_d > 0).all() and (want_w < 0).all()
    w, d = host_update(hostlib, c, 24, 257, wrap, 1, 0, targets=tg)
    np.testing.assert_array_equal(w, want_w)
    # three updates in a row
    c = nc.case(10, 5, "mixed")
    w_ref = w_host = c.weights
    for k in range(3):
        w_ref, d_ref = nr.update(10, c.tuples, 9, w_ref, c.boards, c.meta, c.targets, 9000 + k, 10)
        w_host, d_host = host_update(hostlib, c, 9, 257, w_host, 9000 + k, 10)
        np.testing.assert_array_equal(d_host, d_ref)
        np.testing.assert_array_equal(w_host, w_ref)


@pytest.mark.parametrize("n", nc.SIZES)
def test_search_against_the_reference(hostlib, n):
    tp, shift, w = nc.search_net(n)
    names = ("value", "best", "move_values", "status", "nodes")
    for depth in sh.depths(n):
        s, res = nc.search_reference(n, depth)
        assert set(res.status.tolist()) == {sh.DONE, sh.TERMINATED, sh.NO_MOVE}
        got = host_search(hostlib, s, depth, tp, shift, w, terminal=64)
        for name, g, want in zip(names, got, res.outputs()):
            np.testing.assert_array_equal(g, want, err_msg="%s at depth %d" % (name, depth))
    # a budget small enough to abort some board, not all
    s, res = nc.search_reference(n, 3, nc.BUDGET)
    assert (res.status == sh.ABORTED).any() and (res.status == sh.DONE).any()
    got = host_search(hostlib, s, 3, tp, shift, w, terminal=64, max_nodes=nc.BUDGET)
    for name, g, want in zip(names, got, res.outputs()):
        np.testing.assert_array_equal(g, want, err_msg="%s under a budget" % name)


def test_refusals(hostlib):
    c = nc.case(8, 5, "mixed")
    out = np.full(257, 7, dtype=np.int32)
    w = c.weights.copy()

    def ev(n=8, p=None, R=257, **kw):
        p = nc.params(c.tuples, 0) if p is None else p
        return hostlib.host_ntuple_eval(n, R, ctypes.byref(p), ptr(w), ptr(c.boards), ptr(c.meta), ptr(out), None)

    assert ev() == 0 and not (out == 7).all()
    out[:] = 7
    bad = []
    for field, v in (("tuples", 0), ("tuples", 33), ("value_shift", -1), ("value_shift", 25)):
        p = nc.params(c.tuples, 0)
        setattr(p, field, v)
        bad.append(p)
    for v in (0, 9):
        p = nc.params(c.tuples, 0)
        p.length[1] = v
        bad.append(p)
    for v in (-1, 64):
        p = nc.params(c.tuples, 0)
        p.squares[0][3] = v
        bad.append(p)
    p = nc.params(c.tuples, 0)
    p.squares[0][3] = p.squares[0][0]  # a square twice
    bad.append(p)
    for p in bad:
        assert ev(p=p) == 1
        assert hostlib.host_ntuple_weight_count(8, ctypes.byref(p)) == 0
    assert ev(n=3) == 1 and ev(n=17) == 1 and ev(R=-1) == 1
    assert (out == 7).all()
    p = nc.params(c.tuples, 0)  # fields beyond T and l_t are not read
    p.length[5], p.squares[1][2], p.squares[7][0] = 99, -5, 1000
    assert ev(p=p) == 0
