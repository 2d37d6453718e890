"""oth_puct_pick and oth_puct_reroot's per-board core (csrc/puct.hpp: puct_pick_board,
puct_reroot_board, the text the device kernels run, compiled for the host with
g++: tests/host/puct_play_host.cpp) against the plain Python integers of
tests/puct_play_ref.py: whole games of begin, advances, pick, step, reroot, every
leaf and every output compared after every call.  Every comparison is exact
equality; the workspace starts as garbage."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import family_cases as fc
import puct_play_ref as pp
import puct_ref as pf
import test_puct_host as tph

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "puct_play_host.cpp")
LIB = os.path.join(HERE, "host", "libpuct_play_host.so")


def _stale(lib, src):
    return not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in [src] + tph.HDRS)


@pytest.fixture(scope="module")
def libs():
    """(the search's host library of tests/test_puct_host.py, the self-play calls' own)"""
    for lib, src in ((tph.LIB, tph.SRC), (LIB, SRC)):
        if _stale(lib, src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", lib, src])
    S, L = ctypes.CDLL(tph.LIB), ctypes.CDLL(LIB)
    P, I = ctypes.c_void_p, ctypes.c_int
    S.host_puct_ws_words.argtypes = [I, I, I]
    S.host_puct_ws_words.restype = ctypes.c_uint64
    S.host_puct_begin.argtypes = [I, I, I, P, P, P, P, P, P, P, P]
    S.host_puct_advance.argtypes = [I, I, I, I, P, P, P, I, P, P, P, P]
    S.host_puct_result.argtypes = [I, I, I, P, P, P, P, P, P]
    L.host_puct_pick.argtypes = [I, I, I, P, P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, P]
    L.host_puct_reroot.argtypes = [I, I, I, I, P, P, P, P, P, P, P, P, P, P, P]
    return S, L


ptr = tph.ptr


class HostGame(tph.HostSearch):
    """The host build's search with the two self-play calls."""

    def __init__(self, libs, s, C, T):
        tph.HostSearch.__init__(self, libs[0], s, C, T)
        self.P = libs[1]

    def pick(self, sample, seed, id_key, id_base, counter):
        out = np.full(self.E, 7, dtype=np.int32)
        assert self.P.host_puct_pick(self.n, self.E, self.T, ptr(self.ws), None if sample is None else ptr(sample), seed,
                                     id_key, id_base, counter, ptr(out)) == 0
        return out

    def reroot(self, h, actions, root_priors):
        kept = np.full(self.E, 7, dtype=np.uint8)
        for a in self.leaves():
            a[...] = 7
        actions = np.ascontiguousarray(actions, dtype=np.int32)
        rp = None if root_priors is None else np.ascontiguousarray(root_priors, dtype=np.int32)
        assert self.P.host_puct_reroot(self.n, self.E, self.T, self.C, ptr(self.ws), ptr(h.boards), ptr(h.meta),
                                       ptr(h.legal), ptr(actions), None if rp is None else ptr(rp), ptr(kept),
                                       ptr(self.kind), ptr(self.boards), ptr(self.meta), ptr(self.legal)) == 0
        return kept


def play(hg, game, c, what=""):
    """The game of the reference on a HostGame-like object, everything compared after every call."""
    n, E, S, M, C, T = c
    it = iter(game.leaves)
    tph.same_leaves(hg.leaves(), next(it), what + "begin")
    for m, mv in enumerate(game.moves):
        for i in range(S):
            priors, values = pf.hash_eval(hg.leaves()[1], hg.leaves()[2], n * n)
            hg.advance(priors, values, True)
            tph.same_leaves(hg.leaves(), next(it), what + "move %d advance %d" % (m, i))
        for name, g, w in zip(pf.NAMES, hg.result(), mv["results"]):
            np.testing.assert_array_equal(g, w, err_msg="%smove %d %s" % (what, m, name))
        picks = hg.pick(game.sample, pp.SEED, pp.ID_KEY, 0, mv["counter"])
        np.testing.assert_array_equal(picks, mv["picks"], err_msg="%smove %d picks" % (what, m))
        np.testing.assert_array_equal(hg.pick(None, pp.SEED, pp.ID_KEY, 0, mv["counter"]), mv["results"][2],
                                      err_msg="%smove %d: pick without sample is best" % (what, m))
        kept = hg.reroot(mv["state"], mv["actions"], mv["root_priors"])
        np.testing.assert_array_equal(kept, mv["kept"], err_msg="%smove %d kept" % (what, m))
        tph.same_leaves(hg.leaves(), next(it), what + "move %d reroot" % m)
        np.testing.assert_array_equal(hg.result()[3], mv["used"], err_msg="%smove %d tree_nodes" % (what, m))


@pytest.mark.parametrize("c", pp.CASES, ids=lambda c: pp.CASE_ID % c)
def test_exact_against_the_reference(libs, c):
    s, game = pp.case(c)
    pp.check_case(c, game)
    n, E, S, M, C, T = c
    play(HostGame(libs, s, C, T), game, c)


def test_the_draw_is_keyed_by_the_global_id_and_the_counter(libs):
    """A shard with env_id_base sees the slice of the unsharded draws; another counter, seed or
    id_key gives other draws; sample off draws nothing."""
    c = pp.CASES[1]
    n, E, S, M, C, T = c
    s, game = pp.case(c)
    hg = HostGame(libs, s, C, T)
    for i in range(S):
        priors, values = pf.hash_eval(hg.boards, hg.meta, n * n)
        hg.advance(priors, values, True)
    on = np.ones(E, dtype=np.uint8)
    full = hg.pick(on, 99, 7, 0, 2 ** 40 + 3)
    # the slice of boards 4..8 as a handle of its own with env_id_base = 4 (the same trees: one search a board)
    from oracle import oracle
    t = oracle.State(n, 5)
    t.boards[:], t.meta[:], t.legal[:] = s.boards[4:9], s.meta[4:9], s.legal[4:9]
    part = HostGame(libs, t, C, T)
    for i in range(S):
        priors, values = pf.hash_eval(part.boards, part.meta, n * n)
        part.advance(priors, values, True)
    np.testing.assert_array_equal(part.pick(on[:5], 99, 7, 4, 2 ** 40 + 3), full[4:9])
    np.testing.assert_array_equal(part.pick(on[:5], 99, 3, 8, 2 ** 40 + 3), full[4:9])  # id_key + base is what counts
    others = [hg.pick(on, 99, 7, 0, 2 ** 40 + 4), hg.pick(on, 98, 7, 0, 2 ** 40 + 3), hg.pick(on, 99, 8, 0, 2 ** 40 + 3),
              hg.pick(on, 99, 7, 0, 3)]
    assert all((o != full).any() for o in others)
    np.testing.assert_array_equal(hg.pick(on * 0, 99, 7, 0, 5), hg.result()[2])
    # the sampled squares follow the visits: over many counters every visited child of a board comes up, no other
    visits = hg.result()[0]
    seen = np.zeros_like(visits, dtype=bool)
    for k in range(400):
        a = hg.pick(on, 5, 0, 0, k)
        live = a >= 0
        seen[np.flatnonzero(live), a[live]] = True
    assert not seen[visits == 0].any() and seen[visits >= 3].all()


def test_reroot_to_somewhere_else_is_begin(libs):
    """Actions -1, or a handle on other positions: every board is begun afresh from the handle's
    position, exactly as puct_begin does, and the search goes on as from begin."""
    c = pp.CASES[1]
    n, E, S, M, C, T = c
    s, game = pp.case(c)
    ref = pf.Run(s, 10, C, T)
    for actions, h in ((np.full(E, -1, dtype=np.int32), s), (game.moves[0]["actions"], s)):
        hg = HostGame(libs, s, C, T)
        for i in range(S):
            priors, values = pf.hash_eval(hg.boards, hg.meta, n * n)
            hg.advance(priors, values, True)
        kept = hg.reroot(h, actions, None)
        assert not kept.any()
        tph.same_leaves(hg.leaves(), ref.leaves[0], "reroot")
        for i in range(10):
            priors, values = pf.hash_eval(hg.boards, hg.meta, n * n)
            hg.advance(priors, values, i < 9)
            tph.same_leaves(hg.leaves(), ref.leaves[i + 1], "advance %d after the reroot" % i)
        for name, g, w in zip(pf.NAMES, hg.result(), ref.outputs):
            np.testing.assert_array_equal(g, w, err_msg=name)


@pytest.mark.parametrize("c", [fc.play_case(n) for n in fc.NEW_SIZES], ids=lambda c: pp.CASE_ID % c)
def test_every_other_size_against_the_reference(libs, c):
    """The board sizes puct_play_ref.CASES leaves out: the device's cases of tests/test_gpu_family_sizes.py on the host
    build."""
    assert sorted({k[0] for k in pp.CASES} | set(fc.NEW_SIZES)) == fc.ALL_SIZES
    s, game = pp.case(c)
    fc.check_play_case(c, game)
    n, E, S, M, C, T = c
    play(HostGame(libs, s, C, T), game, c)
