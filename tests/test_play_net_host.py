"""The network's move (csrc/play_net.hpp's shared part -- the argmax key, the
draw's word and target, the cumulative scan: the text the device kernel runs --
compiled for the host with g++: tests/host/play_net_host.cpp) against
tests/play_net_ref.py on the rows of tests/net_cases.py: colours that overlap,
empty and full legal words, bits at or above nn and every meta bit.  Every
comparison is exact equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import net_cases as nc
import net_ref as nr
import play_net_ref as pn
import rng_ref
from oracle import oracle
from test_net_host import load_hostlib, packed, params, ptr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "play_net_host.cpp")
LIB = os.path.join(HERE, "host", "libplay_net_host.so")
HDRS = [os.path.join(ROOT, "gymothelloenv_amd", "csrc", f) for f in ("play_net.hpp", "net.hpp", "bitboard.hpp")]
SEED, ID_BASE = 0xFEDCBA9876543210, 0xFFFFFFF0  # (the ids wrap mod 2^32 inside a case)


@pytest.fixture(scope="module")
def movelib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    P, I, U32, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
    L.host_net_move_rule.argtypes = [I, P, P, P, I, I, U32]
    L.host_net_move_word.argtypes = [U64, U32, U64]
    L.host_net_move_word.restype = U32
    L.host_net_sample_square.argtypes = [I, P, P, U32]
    L.host_net_moves.argtypes = [I, P, I, P, P, P, P, I, U64, U32, P, P]
    return L


def state_of(c):
    s = oracle.State(c.n, c.R)
    s.boards[:], s.meta[:], s.legal[:] = c.boards, c.meta, c.legal
    return s


def expected(c, sample_discs, g):
    """The reference's rule on a case's recorded logits and priors."""
    lg = nr.bits(c.legal, c.nn)
    D = pn.discs(state_of(c))
    u = rng_ref.philox4x32_10(SEED, rng_ref.ids_from(ID_BASE, c.R), g, pn.P_NET_MOVE)[:, 0]
    return np.array([pn.move_rule(c.logits[r], c.priors[r], [int(a) for a in np.flatnonzero(lg[r])], int(D[r]),
                                  sample_discs, u[r]) for r in range(c.R)], dtype=np.int32)


def test_the_draws_word(movelib):
    for seed, gid, g in ((0, 0, 0), (SEED, 0xFFFFFFFF, (1 << 63) + 5), (1, 2, 1 << 32), (2 ** 64 - 1, 7, 2 ** 64 - 1)):
        assert movelib.host_net_move_word(seed, gid, g) == int(rng_ref.philox4x32_10(seed, [gid], g, 7)[0, 0])
    assert movelib.host_net_move_word(5, 6, 7) != int(rng_ref.philox4x32_10(5, [6], 7, 4)[0, 0])  # not puct_pick's


@pytest.mark.parametrize("i", range(len(nc.TABLE)), ids=nc.IDS)
def test_moves_equal_the_reference(movelib, i):
    c = nc.case(i)
    p = params(c.L, c.H, c.shifts, c.policy_shift, c.value_shift)
    blob = packed(load_hostlib(), c, p)
    D = pn.discs(state_of(c))
    mid = int(sorted(D)[c.R // 2])
    g = (np.uint64(1) << np.uint64(33)) + np.arange(c.R, dtype=np.uint64) * np.uint64(3)
    boards, meta, legal = c.boards.copy(), c.meta.copy(), c.legal.copy()
    seen = []
    for sample_discs in (0, 257, mid, mid + 1):
        whole = np.full(c.R + 64, 7, dtype=np.int32)
        out = whole[:c.R]
        assert movelib.host_net_moves(c.n, ctypes.byref(p), c.R, ptr(blob), ptr(boards), ptr(meta), ptr(legal),
                                      sample_discs, SEED, ID_BASE, ptr(g), ptr(out)) == 0
        assert (whole[c.R:] == 7).all()
        np.testing.assert_array_equal(out, expected(c, sample_discs, g), err_msg="sample_discs %d" % sample_discs)
        seen.append(out.copy())
    lg = nr.bits(c.legal, c.nn)
    none = lg.sum(1) == 0
    for out in seen:  # a legal square, or -1 exactly where there is none
        assert ((out == -1) == none).all()
        assert all(lg[r, out[r]] for r in range(c.R) if not none[r])
    if c.R >= 3:
        assert seen[0][1] == -1 and seen[1][1] == -1  # the empty legal words
    # the boundary: a row with D = sample_discs - 1 samples, one with D = sample_discs does not
    at, below = D == mid, D == mid - 1
    np.testing.assert_array_equal(seen[2][at], seen[0][at])
    np.testing.assert_array_equal(seen[3][at], seen[1][at])
    np.testing.assert_array_equal(seen[2][below], seen[1][below])
    if i == 4:  # by the reference alone: the case tells argmax from sampling, and the reference's net_move agrees
        assert (seen[0] != seen[1]).sum() > c.R // 4
        np.testing.assert_array_equal(pn.net_move(c.net, state_of(c), mid, SEED, ID_BASE, g), seen[2])


def test_argmax_ties_pick_the_lowest_square(movelib):
    nn = 100
    stored = np.array([0, 0], dtype=np.uint64)
    for a in (5, 63, 64, 70, 99):
        stored[a >> 6] |= np.uint64(1) << np.uint64(a & 63)
    stored[1] |= np.uint64(1) << np.uint64(40)  # square 104: off the board, never a move
    prior = np.zeros(nn, dtype=np.int32)

    def move(z):
        z = np.asarray(z, dtype=np.int32)
        return movelib.host_net_move_rule(nn, ptr(z), ptr(prior), ptr(stored), 4, 0, 12345)

    z = np.zeros(nn + 1, dtype=np.int32)
    assert move(z) == 5  # the zero network: the lowest legal square
    z[:] = -2 ** 31
    assert move(z) == 5  # ... at the smallest logit too
    z[63], z[64], z[99] = 9, 9, 9
    assert move(z) == 63
    z[70] = 10
    assert move(z) == 70
    z[3] = 2 ** 31 - 1  # not legal
    assert move(z) == 70
    z[99] = 2 ** 31 - 1
    assert move(z) == 99
    none = np.zeros(2, dtype=np.uint64)
    assert movelib.host_net_move_rule(nn, ptr(z), ptr(prior), ptr(none), 4, 0, 1) == -1
    assert movelib.host_net_move_rule(nn, ptr(z), ptr(prior), ptr(none), 4, 257, 1) == -1


def test_every_target_picks_in_proportion(movelib):
    """For a fixed row, sweeping every r in [0, P) picks square a exactly prior[a] times."""
    c = nc.case(4)
    lg = nr.bits(c.legal, c.nn)
    r_ = next(r for r in range(c.R) if 4 <= lg[r].sum() <= 30)
    prior, stored = c.priors[r_].copy(), c.legal[r_].copy()
    legal_sq = np.flatnonzero(lg[r_])
    prior[legal_sq[0]] = prior[legal_sq[2]] = 0  # legal squares of prior 0, the first among them
    P = int(prior[lg[r_] == 1].sum())
    assert 1 <= P <= 65535 + c.nn
    picks = np.bincount([movelib.host_net_sample_square(c.nn, ptr(stored), ptr(prior), r) for r in range(P)],
                        minlength=c.nn)
    np.testing.assert_array_equal(picks, prior)  # a legal square of prior 0 is never drawn
    assert movelib.host_net_sample_square(c.nn, ptr(stored), ptr(prior), P) == -1
    # the rule's target is floor(u P / 2^32): the largest u still draws the last square with a prior
    last = int(np.flatnonzero(prior)[-1])
    z = c.logits[r_].copy()
    assert movelib.host_net_move_rule(c.nn, ptr(z), ptr(prior), ptr(stored), 0, 1, 2 ** 32 - 1) == last
    assert movelib.host_net_move_rule(c.nn, ptr(z), ptr(prior), ptr(stored), 0, 1, 0) == int(np.flatnonzero(prior)[0])


def test_sample_discs_boundary(movelib):
    nn = 16
    stored = np.array([0b0110_0000_0000_0110], dtype=np.uint64)
    z = np.zeros(nn + 1, dtype=np.int32)
    z[13] = 5
    prior = np.zeros(nn, dtype=np.int32)
    prior[1] = 65535  # (not what a network gives for this z: the rule reads what it is handed)
    for sample_discs in (1, 7, 257):
        assert movelib.host_net_move_rule(nn, ptr(z), ptr(prior), ptr(stored), sample_discs - 1, sample_discs, 99) == 1
        if sample_discs < 257:
            assert movelib.host_net_move_rule(nn, ptr(z), ptr(prior), ptr(stored), sample_discs, sample_discs, 99) == 13
    assert movelib.host_net_move_rule(nn, ptr(z), ptr(prior), ptr(stored), 0, 0, 99) == 13
    assert movelib.host_net_move_rule(nn, ptr(z), ptr(prior), ptr(stored), 256, 257, 99) == 1


def test_another_geometry_gives_no_move(movelib):
    c = nc.case(2)
    p = params(c.L, c.H, c.shifts, c.policy_shift, c.value_shift)
    blob = packed(load_hostlib(), c, p)
    other = params(c.L, c.H, c.shifts, c.policy_shift + 1, c.value_shift)
    out = np.full(c.R, 7, dtype=np.int32)
    g = np.zeros(c.R, dtype=np.uint64)
    boards, meta, legal = c.boards.copy(), c.meta.copy(), c.legal.copy()
    assert movelib.host_net_moves(c.n, ctypes.byref(other), c.R, ptr(blob), ptr(boards), ptr(meta), ptr(legal), 0, 1, 0,
                                  ptr(g), ptr(out)) == 2
    assert (out == 7).all()
    for bad in (-1, 258):
        assert movelib.host_net_moves(c.n, ctypes.byref(p), c.R, ptr(blob), ptr(boards), ptr(meta), ptr(legal), bad, 1, 0,
                                      ptr(g), ptr(out)) == 1
