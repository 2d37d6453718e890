"""The play-ntuple core (csrc/play_ntuple.hpp's shared part over csrc/ntuple.hpp, the text
the device kernel runs, compiled for the host with g++: tests/host/play_ntuple_host.cpp)
against the reference of the move T and of the TD target in tests/play_ntuple_ref.py;
NTuplePlayer's validation and the C ABI's bindings.  Every comparison is exact equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ntuple_cases as nc
import play_ntuple_ref as pn
import rng_ref as rr
import search_ref as sh
import solve_ref as sr
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "play_ntuple_host.cpp")
LIB = os.path.join(HERE, "host", "libplay_ntuple_host.so")
HDRS = [os.path.join(ROOT, "gymothelloenv_amd", "csrc", f)
        for f in ("play_ntuple.hpp", "play_search.hpp", "ntuple.hpp", "search.hpp", "root_tasks.hpp", "bitboard.hpp")]
SIZES = [4, 6, 8, 10, 16]
SEED, ID_BASE = 0x123456789ABCDEF, 4000000000  # (a 64-bit key; ids that wrap past 2^32)


def load_movelib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    P, I = ctypes.c_void_p, ctypes.c_int
    L.host_ntuple_move.argtypes = [I, I, P, P, P, P, P, I, I, I, I, ctypes.c_uint64, ctypes.c_uint64, P, P, P, P, P, P]
    return L


@pytest.fixture(scope="module")
def movelib():
    return load_movelib()


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_moves(L, s, p, seed=0, ids=None, g=0, targets=True):
    """(actions, fallbacks, explored, targets) of the host build on State s under policy p."""
    E = s.E
    ids = np.ascontiguousarray(rr.ids_from(0, E) if ids is None else ids).astype(np.uint32)
    g = np.ascontiguousarray(np.broadcast_to(np.asarray(g, dtype=np.uint64), (E,)))
    act, fb, ex = np.full(E, 7, dtype=np.int32), np.full(E, 7, dtype=np.uint8), np.full(E, 7, dtype=np.uint8)
    tg = np.full(E, 7, dtype=np.int32) if targets else None
    w = np.ascontiguousarray(p.weights, dtype=np.int32)
    assert L.host_ntuple_move(s.n, E, ptr(s.boards), ptr(s.meta), ptr(s.legal), ctypes.byref(nc.params(p.tuples, p.shift)),
                              ptr(w), p.depth, p.terminal, p.endgame_empties, p.explore, p.max_nodes, seed, ptr(ids),
                              ptr(g), ptr(act), ptr(fb), ptr(ex), ptr(tg)) == 0
    return act, fb, ex, tg


def policies(n):
    """Black's and white's policy of the move tests: two nets, depth 3 (2 from 10 x 10 on) under
    ntuple_cases.BUDGET against depth 2 without a budget, endgame mode on black's side."""
    tb, sb, wb = nc.search_net(n)
    cw = nc.case(n, 32, "mixed")
    black = pn.pol(tb, sb, wb, depth=2 if n >= 10 else 3, terminal=64, endgame_empties=5, max_nodes=nc.BUDGET)
    white = pn.pol(cw.tuples, 9, cw.weights, depth=2, terminal=1000)
    return black, white


def reference_targets(s, a, done, p):
    nxt = s.copy()
    live = (s.meta & 2) == 0
    _, dn, _ = oracle.step(nxt, 0, np.where(live, a, 0))
    t = pn.targets(s, nxt, dn, p, p)
    kinds = np.where(dn != 0, 0, np.where(((nxt.meta ^ s.meta) & 1) == 0, 2, 1))
    return np.where(done, t, 0).astype(np.int32), kinds


@pytest.mark.parametrize("n", SIZES)
def test_greedy_equivalent_policy(n):
    """GEQ's move is oracle.greedy's on every live board, by the reference alone."""
    s, _ = sh.batch(n, 74)
    act, fb = pn.moves(s, pn.geq(n), pn.geq(n))[:2]
    live = (s.meta & 2) == 0
    assert live.sum() > 50 and not fb.any()
    np.testing.assert_array_equal(act[live], oracle.greedy(s)[live])


@pytest.mark.parametrize("n", SIZES)
def test_moves_and_targets_equal_the_reference(movelib, n):
    s, _ = sh.batch(n, 74)
    black, white = policies(n)
    seen = set()
    for p in (black, white):
        a, f, ex, end, done = pn.moves(s, p, p)
        if p is black:  # by the reference alone: the budget aborts some boards, not all; endgame-mode boards
            assert f.sum() >= 5 and done.sum() >= 5 and end.sum() >= 5, (int(f.sum()), int(done.sum()), int(end.sum()))
        assert (a[[0, 2]] == -1).all() and not f[[0, 2]].any()  # the terminated board and the empty mask
        assert not ex.any()
        want_t, kinds = reference_targets(s, a, done, p)
        seen |= set(kinds[done].tolist())
        got = host_moves(movelib, s, p)
        np.testing.assert_array_equal(got[0], a)
        np.testing.assert_array_equal(got[1], f)
        assert not got[2].any()
        np.testing.assert_array_equal(got[3], want_t)
        assert (np.abs(want_t[done & (kinds == 0)]) == 32768).sum() >= 1
    assert seen == {0, 1, 2}, "the batch holds a game end, a pass and a plain move among its learning rows"
    # without targets: the same moves
    np.testing.assert_array_equal(host_moves(movelib, s, white, targets=False)[0], pn.moves(s, white, white)[0])


@pytest.mark.parametrize("explore", [1, 16384, 40000, 65535, 65536])
@pytest.mark.parametrize("n", [4, 6, 10, 16])
def test_exploration_equals_the_reference(movelib, n, explore):
    s, _ = sh.batch(n, 74)
    p = policies(n)[1]._replace(explore=explore)
    ids = rr.ids_from(ID_BASE, s.E)
    g = (np.arange(s.E, dtype=np.uint64) * np.uint64(977)) + np.uint64((1 << 40) + 5)
    a, f, ex, _, done = pn.moves(s, p, p, SEED, ids, g)
    got = host_moves(movelib, s, p, SEED, ids, g)
    np.testing.assert_array_equal(got[0], a)
    np.testing.assert_array_equal(got[1], f)
    np.testing.assert_array_equal(got[2] != 0, ex)
    np.testing.assert_array_equal(got[3], reference_targets(s, a, done, p)[0])  # (an exploring ply has none)
    wants = ((s.meta & 2) == 0) & sr.legal_rows(s.legal, n * n).any(1)
    if explore == 65536:  # every move is the draw's
        assert (ex == wants).all() and not f.any() and not done.any()
        rows = sr.legal_rows(s.legal, n * n)
        x = rr.philox4x32_10(SEED, ids, g, 8).astype(np.uint64)
        k = (x[:, 1] * rows.sum(1).astype(np.uint64)) >> np.uint64(32)
        np.testing.assert_array_equal(got[0][wants], pn.kth_square(rows, k)[wants])
    elif explore == 16384:
        assert 0 < ex.sum() < wants.sum()
    # another ply, another draw; the same ply, the same draw
    if explore == 40000:
        again = host_moves(movelib, s, p, SEED, ids, g)
        other = host_moves(movelib, s, p, SEED, ids, g + np.uint64(1))
        assert all((x == y).all() for x, y in zip(again, got)) and (other[2] != got[2]).any()


def test_argument_refusals(movelib):
    s, _ = sh.batch(4, 74)
    tp, shift, w = nc.search_net(4)
    E = s.E
    ids, g = rr.ids_from(0, E).astype(np.uint32), np.zeros(E, dtype=np.uint64)
    out = [np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.uint8), np.zeros(E, dtype=np.uint8)]
    good = dict(depth=1, term=64, end=0, explore=0, budget=1)
    for bad in (dict(depth=0), dict(depth=15), dict(term=0), dict(term=32768), dict(end=-1), dict(end=15),
                dict(explore=-1), dict(explore=65537), dict(budget=0), dict(budget=1 << 32)):
        k = dict(good, **bad)
        assert movelib.host_ntuple_move(4, E, ptr(s.boards), ptr(s.meta), ptr(s.legal), ctypes.byref(nc.params(tp, shift)),
                                        ptr(w), k["depth"], k["term"], k["end"], k["explore"], k["budget"], 0, ptr(ids),
                                        ptr(g), ptr(out[0]), ptr(out[1]), ptr(out[2]), None) == -1
    assert not any(o.any() for o in out)


def test_player_validation_and_bindings():
    from gymothelloenv_amd import _lib as L
    P, I32, U64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
    assert L.SIGNATURES["oth_play_ntuple"] == (I32, [P, P, P, I32, P, P, P, P, P, P])
    assert L.SIGNATURES["oth_reset_vs_ntuple"] == (I32, [P, P, P, P, P])
    assert L.SIGNATURES["oth_step_vs_ntuple"] == (I32, [P, P, P, P, P, P, P, P, P])
    assert L.SIGNATURES["oth_ntuple_update_masked"] == (I32, [I32, I32, P, P, U64, P, U64, P, P, P, P, I32, I32, P, P])
    S = L.OthNtuplePolicy
    base = ctypes.sizeof(L.OthNtupleParams)
    assert base == 4 * (1 + 32 + 256 + 1) and base % 8 == 0
    assert [(f, getattr(S, f).offset - base) for f, _ in S._fields_[1:]] == [
        ("plan", 0), ("plan_bytes", 8), ("weights", 16), ("weight_count", 24), ("depth", 32), ("terminal_weight", 36),
        ("endgame_empties", 40), ("explore", 44), ("max_nodes", 48)] and ctypes.sizeof(S) == base + 56
    assert [f for f, _ in L.OthNtupleTd._fields_] == ["boards", "meta", "targets", "learn"]
    assert ctypes.sizeof(L.OthNtupleTd) == 32 and L.OTH_NTUPLE_EXPLORE_ONE == 65536
    header = open(os.path.join(ROOT, "include", "othello_mi355x.h")).read()
    assert "#define OTH_NTUPLE_EXPLORE_ONE 65536" in header
    for name, T in (("oth_ntuple_policy", S), ("oth_ntuple_td", L.OthNtupleTd)):
        body = header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)]
        assert [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.splitlines()[1:] if ";" in ln] == \
            [f for f, _ in T._fields_]
    assert "purpose 8" in header and "RNG_NTUPLE_EXPLORE = 8" in open(
        os.path.join(ROOT, "gymothelloenv_amd", "csrc", "state.hpp")).read()
