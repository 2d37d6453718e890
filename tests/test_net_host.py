"""The network's core (csrc/net.hpp: the packed layout, the pack step and the row
logic that the device kernel takes its layout and per-element steps from, compiled
for the host with g++: tests/host/net_host.cpp) against the numpy and Python
integers of tests/net_ref.py on every case of tests/net_cases.py, with guard words
behind every buffer.  Every comparison is exact equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import net_cases as nc
import net_ref as nr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "net_host.cpp")
LIB = os.path.join(HERE, "host", "libnet_host.so")
HDRS = [os.path.join(ROOT, "gymothelloenv_amd", "csrc", f) for f in ("net.hpp", "bitboard.hpp")]
GUARD = 64  # bytes or elements behind a buffer that no call may touch


class Params(ctypes.Structure):
    _fields_ = [("layers", ctypes.c_int32), ("width", ctypes.c_int32), ("shift", ctypes.c_int32 * 4),
                ("policy_shift", ctypes.c_int32), ("value_shift", ctypes.c_int32)]


def params(L, H, shifts, policy_shift, value_shift):
    sh = list(shifts) + [0] * (4 - len(shifts))
    return Params(L, H, (ctypes.c_int32 * 4)(*sh), policy_shift, value_shift)


def load_hostlib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    P, I = ctypes.c_void_p, ctypes.c_int
    L.host_net_exp2.argtypes = [I]
    L.host_net_exp2.restype = ctypes.c_uint32
    L.host_net_blob_bytes.argtypes = [I, P]
    L.host_net_blob_bytes.restype = ctypes.c_uint64
    L.host_net_pack.argtypes = [I, P, P, P, P]
    L.host_net_eval.argtypes = [I, P, I, P, P, P, P, P, P, P]
    return L


@pytest.fixture(scope="module")
def hostlib():
    return load_hostlib()


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def guarded(shape, dtype, fill=7):
    """(the whole buffer, the view a call gets): GUARD elements of `fill` behind the view."""
    count = int(np.prod(shape))
    whole = np.full(count + GUARD, fill, dtype=dtype)
    return whole, whole[:count].reshape(shape)


def packed(L, c, p):
    """A case's blob, packed by the host build into a buffer of exactly the reported size."""
    size = int(L.host_net_blob_bytes(c.n, ctypes.byref(p)))
    assert size == nc.blob_bytes(c.n, c.L, c.H)
    whole, blob = guarded((size,), np.uint8, 0xA5)
    w, b = nc.flat_weights(c)
    assert L.host_net_pack(c.n, ctypes.byref(p), ptr(w), ptr(b), ptr(blob)) == 0
    assert (whole[size:] == 0xA5).all()
    return blob


def test_exp2_table(hostlib):
    assert [hostlib.host_net_exp2(f) for f in range(256)] == nr.EXP2
    assert (nr.EXP2[0], nr.EXP2[1], nr.EXP2[255]) == (1073741824, 1070838486, 538326517)


@pytest.mark.parametrize("i", range(len(nc.TABLE)), ids=nc.IDS)
def test_exact_against_the_reference(hostlib, i):
    c = nc.case(i)
    p = params(c.L, c.H, c.shifts, c.policy_shift, c.value_shift)
    blob = packed(hostlib, c, p)
    pw, priors = guarded((c.R, c.nn), np.int32)
    vw, values = guarded((c.R,), np.int32)
    lw, logits = guarded((c.R, c.nn + 1), np.int32)
    boards, meta, legal = c.boards.copy(), c.meta.copy(), c.legal.copy()
    assert hostlib.host_net_eval(c.n, ctypes.byref(p), c.R, ptr(blob), ptr(boards), ptr(meta), ptr(legal), ptr(priors),
                                 ptr(values), ptr(logits)) == 0
    np.testing.assert_array_equal(logits, c.logits)
    np.testing.assert_array_equal(values, c.values)
    np.testing.assert_array_equal(priors, c.priors)
    for whole, view in ((pw, priors), (vw, values), (lw, logits)):
        assert (whole[view.size:] == 7).all()
    # without the logits: the same priors and values
    p2, v2 = np.full_like(priors, 7), np.full_like(values, 7)
    assert hostlib.host_net_eval(c.n, ctypes.byref(p), c.R, ptr(blob), ptr(boards), ptr(meta), ptr(legal), ptr(p2),
                                 ptr(v2), None) == 0
    assert (p2 == priors).all() and (v2 == values).all()


def test_what_the_cases_cover():
    """The properties the table is there for hold of the reference's own outputs."""
    by = dict(zip(nc.FLAVOUR, range(len(nc.TABLE))))
    flat = nc.case(by["flat"])
    lg = nr.bits(flat.legal, flat.nn)
    for r in range(flat.R):  # policy_shift 24: k legal squares get (65535 + k // 2) // k each
        k = int(lg[r].sum())
        want = np.where(lg[r] == 1, (65535 + k // 2) // k if k else 0, 0)
        np.testing.assert_array_equal(flat.priors[r], want)
    gaps = nc.case(by["gaps"])
    lg = nr.bits(gaps.legal, gaps.nn)
    assert ((gaps.priors == 0) & (lg == 1)).any(), "no legal square with an exact 0"
    high = nc.case(by["high"])
    assert abs(high.logits).max() >= nr.BIAS_MAX and (abs(high.values) == 32768).all()
    for i in range(len(nc.TABLE)):
        c = nc.case(i)
        lg = nr.bits(c.legal, c.nn)
        assert (c.priors[lg == 0] == 0).all()
        rows = lg.sum(axis=1) > 0
        assert (abs(c.priors[rows].sum(axis=1) - 65535) <= c.nn).all()  # each prior is rounded once
        assert (c.priors[~rows] == 0).all()
        if c.R >= 3:
            assert not rows[1] and lg[2].all()
    mixed = nc.case(4)
    assert len(set(mixed.priors[mixed.priors > 0].tolist())) > 50 and len(set(mixed.values.tolist())) > 20


def test_rows_are_independent_and_high_bits_are_not_read(hostlib):
    c = nc.case(5)  # N = 9: 81 squares, 47 bits of the second word off the board
    p = params(c.L, c.H, c.shifts, c.policy_shift, c.value_shift)
    blob = packed(hostlib, c, p)
    off = ~np.uint64(0) << np.uint64(c.nn - 64)
    boards, legal = c.boards.copy(), c.legal.copy()
    boards[:, 1] ^= off
    boards[:, 3] ^= off
    legal[:, 1] ^= off
    meta = c.meta ^ np.uint16(0xFFFE)
    order = np.arange(c.R)[::-1].copy()
    b2, m2, l2 = boards[order].copy(), meta[order].copy(), legal[order].copy()
    priors, values = np.full((c.R, c.nn), 7, np.int32), np.full(c.R, 7, np.int32)
    assert hostlib.host_net_eval(c.n, ctypes.byref(p), c.R, ptr(blob), ptr(b2), ptr(m2), ptr(l2), ptr(priors),
                                 ptr(values), None) == 0
    np.testing.assert_array_equal(priors, c.priors[order])
    np.testing.assert_array_equal(values, c.values[order])


def test_another_geometry_writes_nothing(hostlib):
    c = nc.case(2)
    p = params(c.L, c.H, c.shifts, c.policy_shift, c.value_shift)
    blob = packed(hostlib, c, p)
    priors, values = np.full((c.R, c.nn), 7, np.int32), np.full(c.R, 7, np.int32)
    boards, meta, legal = c.boards.copy(), c.meta.copy(), c.legal.copy()
    for other in (params(c.L, c.H, c.shifts, c.policy_shift + 1, c.value_shift),
                  params(c.L, c.H, [c.shifts[0] + 1], c.policy_shift, c.value_shift),
                  params(c.L, 64, c.shifts, c.policy_shift, c.value_shift)):
        assert hostlib.host_net_eval(c.n, ctypes.byref(other), c.R, ptr(blob), ptr(boards), ptr(meta), ptr(legal),
                                     ptr(priors), ptr(values), None) == 2
        assert (priors == 7).all() and (values == 7).all()


def test_pack_rejects_what_is_out_of_range(hostlib):
    c = nc.case(0)
    w, b = nc.flat_weights(c)
    good = params(c.L, c.H, c.shifts, c.policy_shift, c.value_shift)
    blob = np.zeros(nc.blob_bytes(c.n, c.L, c.H), np.uint8)
    for bad in (params(0, 64, [], 0, 0), params(5, 64, [0] * 4, 0, 0), params(1, 32, [0], 0, 0),
                params(1, 96, [0], 0, 0), params(1, 576, [0], 0, 0), params(1, 64, [25], 0, 0),
                params(1, 64, [-1], 0, 0), params(1, 64, [0], 25, 0), params(1, 64, [0], 0, -1)):
        assert hostlib.host_net_blob_bytes(4, ctypes.byref(bad)) == 0
        assert hostlib.host_net_pack(4, ctypes.byref(bad), ptr(w), ptr(b), ptr(blob)) == 1
    assert hostlib.host_net_blob_bytes(3, ctypes.byref(good)) == 0 and hostlib.host_net_blob_bytes(17, ctypes.byref(good)) == 0
    for at, v in ((0, 2 ** 30 + 1), (b.size - 1, -2 ** 30 - 1)):
        b2 = b.copy()
        b2[at] = v
        assert hostlib.host_net_pack(4, ctypes.byref(good), ptr(w), ptr(b2), ptr(blob)) == 2
    assert hostlib.host_net_pack(4, ctypes.byref(good), ptr(w), ptr(b), ptr(blob)) == 0
