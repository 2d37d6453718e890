"""The conv net's move (csrc/play_net.hpp's shared part -- the argmax key, the draw's
word and target, the cumulative scan -- over csrc/cnet.hpp's cnet_row, compiled for
the host with g++: tests/host/play_cnet_host.cpp) against play_net_ref.net_move over
cnet_ref on the rows of two cnet_cases entries, a C = 64 one and a C = 128 one.
Every comparison is exact equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cnet_cases as cc
import net_ref as nr
import play_net_ref as pn
from oracle import oracle
from test_cnet_host import case_params, guarded, ptr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "play_cnet_host.cpp")
LIB = os.path.join(HERE, "host", "libplay_cnet_host.so")
HDRS = [os.path.join(ROOT, "gymothelloenv_amd", "csrc", f) for f in ("play_cnet.hpp", "play_net.hpp", "cnet.hpp", "net.hpp",
                                                                     "bitboard.hpp")]
SEED, ID_BASE = 0xFEDCBA9876543210, 0xFFFFFFF0  # (the ids wrap mod 2^32 inside a case)
CASES = [cc.TABLE.index((5, 17, 1, 64)), cc.TABLE.index((6, 15, 2, 128))]


@pytest.fixture(scope="module")
def movelib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    P, I, U32, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
    L.host_cnet_moves.argtypes = [I, P, I, P, P, P, P, I, U64, U32, P, P]
    L.host_play_cnet_blob_bytes.argtypes = [I, P]
    L.host_play_cnet_blob_bytes.restype = U64
    L.host_play_cnet_pack.argtypes = [I, P, P, P, P]
    return L


def state_of(c):
    s = oracle.State(c.n, c.R)
    s.boards[:], s.meta[:], s.legal[:] = c.boards, c.meta, c.legal
    return s


def packed(L, c, p):
    size = int(L.host_play_cnet_blob_bytes(c.n, ctypes.byref(p)))
    assert size == cc.blob_bytes(c.n, c.B, c.C)
    whole, blob = guarded((size,), np.uint8, 0xA5)
    w, b = cc.flat_weights(c)
    assert L.host_play_cnet_pack(c.n, ctypes.byref(p), ptr(w), ptr(b), ptr(blob)) == 0
    assert (whole[size:] == 0xA5).all()
    return blob


@pytest.mark.parametrize("i", CASES, ids=[cc.IDS[i] for i in CASES])
def test_moves_equal_the_reference(movelib, i):
    c = cc.case(i)
    p = case_params(c)
    blob = packed(movelib, c, p)
    s = state_of(c)
    D = pn.discs(s)
    mid = int(sorted(D)[c.R // 2])  # the rows' median disc count: rows on both sides of it
    assert (D < mid).any() and (D >= mid).any()
    g = (np.uint64(1) << np.uint64(33)) + np.arange(c.R, dtype=np.uint64) * np.uint64(3)
    boards, meta, legal = c.boards.copy(), c.meta.copy(), c.legal.copy()
    seen = []
    for sample_discs in (0, 257, mid):
        whole, out = guarded((c.R,), np.int32)
        assert movelib.host_cnet_moves(c.n, ctypes.byref(p), c.R, ptr(blob), ptr(boards), ptr(meta), ptr(legal),
                                       sample_discs, SEED, ID_BASE, ptr(g), ptr(out)) == 0
        assert (whole[c.R:] == 7).all()
        np.testing.assert_array_equal(out, pn.net_move(c.net, s, sample_discs, SEED, ID_BASE, g),
                                      err_msg="sample_discs %d" % sample_discs)
        seen.append(out.copy())
    lg = nr.bits(c.legal, c.nn)
    none = lg.sum(1) == 0
    assert none.any() and not none.all()
    for out in seen:  # a legal square, or -1 exactly where there is none
        assert ((out == -1) == none).all()
        assert all(lg[r, out[r]] for r in range(c.R) if not none[r])
    # by the reference alone: the case tells argmax from sampling, and the boundary falls between rows
    assert (seen[0] != seen[1]).any()
    np.testing.assert_array_equal(seen[2][D >= mid], seen[0][D >= mid])
    np.testing.assert_array_equal(seen[2][D < mid], seen[1][D < mid])


def test_another_geometry_gives_no_move(movelib):
    c = cc.case(CASES[0])
    p = case_params(c)
    blob = packed(movelib, c, p)
    out = np.full(c.R, 7, dtype=np.int32)
    g = np.zeros(c.R, dtype=np.uint64)
    boards, meta, legal = c.boards.copy(), c.meta.copy(), c.legal.copy()
    for other in (case_params(c, policy_shift=c.policy_shift + 1), case_params(c, shifts=[c.shifts[0], c.shifts[1] + 1])):
        assert movelib.host_cnet_moves(c.n, ctypes.byref(other), c.R, ptr(blob), ptr(boards), ptr(meta), ptr(legal), 0, 1,
                                       0, ptr(g), ptr(out)) == 2
        assert (out == 7).all()
    for bad in (-1, 258):
        assert movelib.host_cnet_moves(c.n, ctypes.byref(p), c.R, ptr(blob), ptr(boards), ptr(meta), ptr(legal), bad, 1, 0,
                                       ptr(g), ptr(out)) == 1
