"""The batch calls' core (csrc/puct.hpp: K leaves a board per launch under virtual
loss, the text the device kernels run, compiled for the host with g++:
tests/host/puct_batch_host.cpp) against the plain Python integers of
tests/puct_batch_ref.py, after begin and after every launch.  Every comparison
is exact equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import family_cases as fc
import puct_batch_ref as pb
import puct_ref as pf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "puct_batch_host.cpp")
LIB = os.path.join(HERE, "host", "libpuct_batch_host.so")
HDRS = [os.path.join(ROOT, "gymothelloenv_amd", "csrc", f)
        for f in ("puct.hpp", "mcts.hpp", "root_tasks.hpp", "bitboard.hpp")]


@pytest.fixture(scope="module")
def hostlib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    P, I = ctypes.c_void_p, ctypes.c_int
    L.host_puct_batch_ws_words.argtypes = [I, I, I, I]
    L.host_puct_batch_ws_words.restype = ctypes.c_uint64
    L.host_puct_plain_ws_words.argtypes = [I, I, I]
    L.host_puct_plain_ws_words.restype = ctypes.c_uint64
    L.host_puct_begin_batch.argtypes = [I, I, I, I, P, P, P, P, P, P, P, P]
    L.host_puct_advance_batch.argtypes = [I, I, I, I, I, P, P, P, I, P, P, P, P]
    L.host_puct_reroot_batch.argtypes = [I, I, I, I, I, P, P, P, P, P, P, P, I, P, P, P, P]
    L.host_puct_batch_result.argtypes = [I, I, I, P, P, P, P, P, P, P]
    L.host_puct_plain_advance.argtypes = [I, I, I, I, P, P, P]
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


GUARD = 64  # words behind the workspace that no call may touch


class HostSearch(object):
    """The batch calls of the host build, on a workspace of garbage of exactly the reported size."""

    def __init__(self, L, s, C, T, K):
        self.L, self.n, self.E, self.C, self.T, self.K, self.nn = L, s.n, s.E, C, T, K, s.n * s.n
        W, R = s.W, s.E * K
        self.words = int(L.host_puct_batch_ws_words(s.n, s.E, T, K))
        self.ws = np.full(self.words + GUARD, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        self.kind = np.full(R, 7, dtype=np.uint8)
        self.boards = np.full((R, 2 * W), 7, dtype=np.uint64)
        self.meta = np.full(R, 7, dtype=np.uint16)
        self.legal = np.full((R, W), 7, dtype=np.uint64)
        assert L.host_puct_begin_batch(s.n, s.E, T, K, ptr(s.boards), ptr(s.meta), ptr(s.legal), ptr(self.ws),
                                       *[ptr(a) for a in self.leaves()]) == 0

    def leaves(self):
        return self.kind, self.boards, self.meta, self.legal

    def refill(self):
        for a in self.leaves():
            a[...] = 7

    def advance(self, priors, values, sim_limit):
        priors, values = np.ascontiguousarray(priors, dtype=np.int32), np.ascontiguousarray(values, dtype=np.int32)
        assert priors.size == self.E * self.K * self.nn and values.size == self.E * self.K
        self.refill()
        assert self.L.host_puct_advance_batch(self.n, self.E, self.T, self.K, self.C, ptr(self.ws), ptr(priors),
                                              ptr(values), sim_limit, *[ptr(a) for a in self.leaves()]) == 0

    def reroot(self, s, actions, root_priors, sim_limit):
        actions = np.ascontiguousarray(actions, dtype=np.int32)
        rp = None if root_priors is None else np.ascontiguousarray(root_priors, dtype=np.int32)
        kept = np.full(self.E, 7, dtype=np.uint8)
        self.refill()
        assert self.L.host_puct_reroot_batch(self.n, self.E, self.T, self.K, self.C, ptr(self.ws), ptr(s.boards),
                                             ptr(s.meta), ptr(s.legal), ptr(actions), ptr(rp), ptr(kept), sim_limit,
                                             *[ptr(a) for a in self.leaves()]) == 0
        return kept

    def result(self):
        E, nn = self.E, self.nn
        out = (np.full((E, nn), 7, dtype=np.int32), np.full((E, nn), 7, dtype=np.int64), np.full(E, 7, dtype=np.int32),
               np.full(E, 7, dtype=np.int32), np.full(E, 7, dtype=np.uint8), np.full(E, 7, dtype=np.int32))
        assert self.L.host_puct_batch_result(self.n, E, self.T, ptr(self.ws), *[ptr(a) for a in out]) == 0
        return out[:5], out[5]

    def guard_untouched(self):
        return (self.ws[self.words:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()


def same_leaves(got, want, what):
    for name, g, w in zip(pf.LEAF_NAMES, got, want):
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (what, name))


def drive(hs, run, sims, what):
    """The whole search against the reference Run, launch by launch."""
    same_leaves(hs.leaves(), run.leaves[0], what + " begin")
    for i in range(len(run.leaves) - 1):
        if i in run.mid:  # result and pick in mid-search equal the reference's and change nothing
            before = hs.ws.copy()
            res, picks = hs.result()
            for name, g, w in zip(pf.NAMES, res, run.mid[i][0]):
                np.testing.assert_array_equal(g, w, err_msg="%s mid %d %s" % (what, i, name))
            np.testing.assert_array_equal(picks, run.mid[i][1])
            assert (hs.ws == before).all()
        priors, values = pf.hash_eval(hs.boards, hs.meta, hs.nn)
        hs.advance(priors, values, sims)
        same_leaves(hs.leaves(), run.leaves[i + 1], "%s launch %d" % (what, i))
    assert not hs.kind.any() and hs.guard_untouched()
    for name, g, w in zip(pf.NAMES, hs.result()[0], run.outputs):
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (what, name))


@pytest.mark.parametrize("c", pb.CASES, ids=lambda c: pb.CASE_ID % c)
def test_exact_against_the_reference(hostlib, c):
    s, run = pb.case(c)
    pb.check_case(c, run)
    n, E, sims, C, T, K = c
    drive(HostSearch(hostlib, s, C, T, K), run, sims, pb.CASE_ID % c)


@pytest.mark.parametrize("c", pb.K1_CASES, ids=lambda c: pf.CASE_ID % c)
def test_k1_is_the_plain_search(hostlib, c):
    """K = 1 against puct_ref.Run, the plain calls' reference: the leaves after every launch and the outputs;
    and the batch reference with K = 1 is that reference."""
    n, E, sims, C, T = c
    s = pb.mr.positions(n, E)
    plain = pf.Run(s.copy(), sims, C, T)
    ref = pb.Run(s.copy(), sims, C, T, 1)
    assert len(ref.leaves) == len(plain.leaves) == sims + 1
    for a, b in zip(ref.leaves, plain.leaves):
        same_leaves(a, b, "the references")
    hs = HostSearch(hostlib, s, C, T, 1)
    same_leaves(hs.leaves(), plain.leaves[0], "begin")
    for i in range(sims):
        priors, values = pf.hash_eval(hs.boards, hs.meta, n * n)
        hs.advance(priors, values, sims)
        same_leaves(hs.leaves(), plain.leaves[i + 1], "advance %d" % i)
    for name, g, w in zip(pf.NAMES, hs.result()[0], plain.outputs):
        np.testing.assert_array_equal(g, w, err_msg=name)


def test_self_play_against_the_reference(hostlib):
    """Moves of launches, result, pick and reroot_batch (root priors on odd moves, leaves pending at the
    re-root on odd moves) against puct_batch_ref.Game, with kept and tree_nodes."""
    for c in ((8, 9, 30, 3, 320, 4096, 4), (8, 12, 40, 3, 320, 64, 8), (10, 8, 20, 2, 320, 4096, 3)):
        n, E, S, M, C, T, K = c
        s, g = pb.game(c)
        assert g.counters["kept"] > 0 and g.counters["fresh"] > 0 and g.counters["priors_set"] > 0
        hs = HostSearch(hostlib, s, C, T, K)
        it = iter(g.leaves)
        same_leaves(hs.leaves(), next(it), "begin")
        for m, mv in enumerate(g.moves):
            for i in range(mv["launches"]):
                priors, values = pf.hash_eval(hs.boards, hs.meta, n * n)
                hs.advance(priors, values, mv["limit"])
                same_leaves(hs.leaves(), next(it), "move %d launch %d" % (m, i))
            res, _ = hs.result()
            for name, a, b in zip(pf.NAMES, res, mv["results"]):
                np.testing.assert_array_equal(a, b, err_msg="move %d %s" % (m, name))
            kept = hs.reroot(mv["state"], mv["actions"], mv["root_priors"], S * (m + 2))
            np.testing.assert_array_equal(kept, mv["kept"])
            same_leaves(hs.leaves(), next(it), "move %d reroot" % m)
            np.testing.assert_array_equal(hs.result()[0][3], mv["used"])
        assert hs.guard_untouched()


def test_families_and_tags(hostlib):
    """A batch call with another K does nothing; a plain advance on a batch workspace stays inside it and
    does nothing to a board (its header's kind is NONE); the sizes nest."""
    c = pb.CASES[3]
    n, E, sims, C, T, K = c
    s, run = pb.case(c)
    L = hostlib
    assert L.host_puct_batch_ws_words(n, E, T, 1) >= L.host_puct_plain_ws_words(n, E, T) + 2
    sizes = [L.host_puct_batch_ws_words(n, E, T, k) for k in range(1, 65)]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    hs = HostSearch(L, s, C, T, K)
    priors, values = pf.hash_eval(hs.boards, hs.meta, n * n)
    hs.advance(priors, values, sims)
    before = hs.ws.copy()
    other = HostSearch.__new__(HostSearch)
    other.__dict__.update(hs.__dict__)
    other.K = K - 1
    other.kind, other.boards, other.meta, other.legal = (a[:E * (K - 1)].copy() for a in hs.leaves())
    other.advance(priors[:E * (K - 1)], values[:E * (K - 1)], sims)
    assert (hs.ws == before).all() and (other.kind == 7).all()  # another K: nothing is done
    assert L.host_puct_plain_advance(n, E, T, C, ptr(hs.ws), ptr(priors), ptr(values)) == 0
    plain_words = int(L.host_puct_plain_ws_words(n, E, T))
    changed = np.flatnonzero(hs.ws != before)
    assert changed.size == 0 or changed.max() < plain_words
    # the trees and the headers are as they were: only the plain calls' own leaf arrays may differ
    W = s.W
    lo, hi = 2 + 2 * E, 2 + 2 * E + 3 * W * E + (E + 3) // 4
    assert ((changed >= lo) & (changed < hi)).all()


@pytest.mark.parametrize("c", [fc.batch_case(n) for n in fc.NEW_SIZES] + [fc.BATCH_WIDE], ids=lambda c: pb.CASE_ID % c)
def test_every_other_size_against_the_reference(hostlib, c):
    """The board sizes puct_batch_ref.CASES leaves out: the device's cases of tests/test_gpu_family_sizes.py on the host
    build."""
    assert sorted({k[0] for k in pb.CASES} | set(fc.NEW_SIZES)) == fc.ALL_SIZES
    s, run, census = fc.batch_run(c)
    fc.check_batch_case(c, run, census)
    n, E, sims, C, T, K = c
    drive(HostSearch(hostlib, s, C, T, K), run, sims, pb.CASE_ID % c)
