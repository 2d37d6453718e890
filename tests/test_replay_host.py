"""The replay store's core (csrc/replay.hpp: the text the device kernels run,
compiled for the host with g++: tests/host/replay_host.cpp) against the plain
Python integers of tests/replay_ref.py, after every call, on a workspace of
garbage of exactly the reported size with guard words behind it.  Every
comparison is exact equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import replay_cases as rc
import replay_ref as rr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "replay_host.cpp")
LIB = os.path.join(HERE, "host", "libreplay_host.so")
HDRS = [os.path.join(ROOT, "gymothelloenv_amd", "csrc", f) for f in ("replay.hpp", "bitboard.hpp")]


def load_hostlib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    P, I, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    L.host_replay_ws_words.argtypes = [I, I, I, I]
    L.host_replay_ws_words.restype = U64
    L.host_replay_sigma.argtypes = [I, I, I]
    L.host_replay_begin.argtypes = [I, I, I, I, P]
    L.host_replay_append.argtypes = [I, I, I, I, P, P, P, P, P, P]
    L.host_replay_label.argtypes = [I, I, I, I, P, P, P]
    L.host_replay_counts.argtypes = [I, I, I, I, P, P]
    L.host_replay_batch.argtypes = [I, I, I, I, P, I, P, P, I, U64, ctypes.c_uint32, U64] + [P] * 8
    L.host_symmetry_masks.argtypes = [I, I, I, P, P, P]
    return L


@pytest.fixture(scope="module")
def hostlib():
    return load_hostlib()


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


GUARD = 64  # words behind the workspace that no call may touch
FILL = 0xA5A5A5A5A5A5A5A5


class HostStore(object):
    """The calls of the host build, on a workspace of garbage of exactly the reported size."""

    def __init__(self, L, n, E, H, B, begin=True):
        self.L, self.n, self.E, self.H, self.B, self.W, self.nn = L, n, E, H, B, rr.nwords(n), n * n
        self.words = int(L.host_replay_ws_words(n, E, H, B))
        self.ws = np.full(self.words + GUARD, FILL, dtype=np.uint64)
        self.geo = (n, E, H, B)
        if begin:
            assert L.host_replay_begin(*self.geo, ptr(self.ws)) == 0

    def append(self, s, visits, skip=None):
        visits = np.ascontiguousarray(visits, dtype=np.int32)
        assert self.L.host_replay_append(*self.geo, ptr(self.ws), ptr(s.boards), ptr(s.meta), ptr(s.legal), ptr(visits),
                                         ptr(skip)) == 0

    def label(self, rewards, dones):
        rewards = np.ascontiguousarray(rewards, dtype=np.int32)
        dones = np.ascontiguousarray(dones, dtype=np.uint8)
        assert self.L.host_replay_label(*self.geo, ptr(self.ws), ptr(rewards), ptr(dones)) == 0

    def counts(self):
        out = np.full(3, 7, dtype=np.int64)
        assert self.L.host_replay_counts(*self.geo, ptr(self.ws), ptr(out)) == 0
        return out

    def outputs(self, cnt, only=None):
        W, nn = self.W, self.nn
        out = [np.full(cnt, 7, dtype=np.uint8), np.full((cnt, 2 * W), 7, dtype=np.uint64),
               np.full(cnt, 7, dtype=np.uint16), np.full((cnt, W), 7, dtype=np.uint64),
               np.full((cnt, nn), 7, dtype=np.int32), np.full(cnt, 7, dtype=np.int32), np.full(cnt, 7, dtype=np.int32),
               np.full(cnt, 7, dtype=np.uint8)]
        return [a if only is None or k in only else None for k, a in zip(rr.NAMES, out)]

    def gather(self, rows, sym=None, only=None):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        sym = None if sym is None else np.ascontiguousarray(sym, dtype=np.uint8)
        out = self.outputs(rows.size, only)
        assert self.L.host_replay_batch(*self.geo, ptr(self.ws), rows.size, ptr(rows), ptr(sym), 0, 0, 0, 0,
                                        *[ptr(a) for a in out]) == 0
        return out

    def sample(self, cnt, augment, seed, id_key, counter, only=None):
        out = self.outputs(cnt, only)
        assert self.L.host_replay_batch(*self.geo, ptr(self.ws), cnt, None, None, int(augment), seed, id_key, counter,
                                        *[ptr(a) for a in out]) == 0
        return out

    def guard_untouched(self):
        return (self.ws[self.words:] == np.uint64(FILL)).all()


# (n, E, H, flags, moves, every): H = 3 wraps a game's ring many times; 37 x 31 = 1,147 rows cross the rank
# step's 1,024-row chunk; 81 squares straddle a word
CASES = [(4, 5, 3, 0, 16, 1), (4, 5, 3, 4, 30, 1), (8, 5, 3, 4 | 2, 70, 8), (9, 5, 3, 2, 60, 8), (8, 37, 31, 4, 70, 16),
         (4, 37, 31, 4 | 2, 40, 8), (12, 5, 3, 4, 30, 10), (16, 5, 3, 0, 24, 12), (6, 3, 4, 1, 40, 4)]
CASE_ID = "n%d-E%d-H%d-flags%d-moves%d-every%d"


@pytest.mark.parametrize("c", CASES, ids=lambda c: CASE_ID % c)
def test_exact_against_the_reference(hostlib, c):
    n, E, H, flags, moves, every = c
    B = E * H + 4
    hs, ref = HostStore(hostlib, n, E, H, B), rr.Store(n, E, H)
    rc.check_store(hs, ref, "begin")
    recorded, finished, labelled = rc.play(hs, ref, rc.OracleGame(n, E, flags, 11), moves, 5, CASE_ID % c, every)
    assert recorded > 0
    if n <= 8:
        assert finished > 0 and labelled > 0, "no game ended"
    if H == 3:
        assert max(ref.count) > 2 * H, "the ring did not wrap"
    # the sample: the rank step over every chunk, with and without the symmetries, and a narrow batch
    for augment, seed, id_key, counter in ((1, 99, 0, 0), (0, 2 ** 64 - 1, 2 ** 32 - 3, 2 ** 63 + 5)):
        want = ref.sample(B, augment, seed, id_key, counter)
        rc.same_batch(hs.sample(B, augment, seed, id_key, counter), want.arrays(), "sample")
        rc.same_batch(hs.sample(B, augment, seed, id_key, counter, only=("visits", "rows")), want.arrays(), "sample")
    assert hs.guard_untouched()


def test_sample_of_few_rows(hostlib):
    """M = 0 gives EMPTY rows and -1; M = 1 gives that row every time; a board with no record labels nothing."""
    n, E, H, B = 8, 37, 31, 64
    hs, ref = HostStore(hostlib, n, E, H, B), rr.Store(n, E, H)
    rc.same_batch(hs.sample(B, 1, 3, 4, 5), ref.sample(B, 1, 3, 4, 5).arrays(), "M = 0")
    assert (hs.sample(B, 1, 3, 4, 5)[6] == -1).all()
    game = rc.OracleGame(n, E, 0, 1)
    visits = np.zeros((E, n * n), dtype=np.int32)
    visits[36] = 3  # only the last board records: row 36 * 31 = 1116, in the second chunk
    for impl in (hs, ref):
        impl.append(game.state(), visits)
        impl.label(np.full(E, 2 ** 20, dtype=np.int32), np.ones(E, dtype=np.uint8))
    np.testing.assert_array_equal(hs.counts(), [E * H - 1, 0, 1])
    got = hs.sample(B, 1, 3, 4, 5)
    rc.same_batch(got, ref.sample(B, 1, 3, 4, 5).arrays(), "M = 1")
    assert (got[6] == 36 * H).all() and (got[5] == 32768).all() and len(set(got[7].tolist())) > 1
    assert hs.guard_untouched()


def test_another_geometry_does_nothing(hostlib):
    """No begin, or a begin of another H or B: append, label, counts, gather and sample leave everything alone."""
    n, E, H, B = 6, 3, 4, 16
    game = rc.OracleGame(n, E, 0, 1)
    visits = np.ones((E, n * n), dtype=np.int32)
    for hs in (HostStore(hostlib, n, E, H, B, begin=False), HostStore(hostlib, n, E, H, B)):
        if hs.ws[0] != np.uint64(FILL):  # begun: call it with another geometry on the same memory
            hs.geo = (n, E, H, B - 1)
        before = hs.ws.copy()
        hs.append(game.state(), visits)
        hs.label(np.ones(E, dtype=np.int32), np.ones(E, dtype=np.uint8))
        assert (hs.counts() == 7).all()
        assert all((a == 7).all() for a in hs.gather(np.arange(4)))
        assert all((a == 7).all() for a in hs.sample(4, 1, 0, 0, 0))
        assert (hs.ws == before).all()


def test_a_byte_copy_is_a_checkpoint(hostlib):
    n, E, H, B = 8, 5, 3, 19
    hs, ref = HostStore(hostlib, n, E, H, B), rr.Store(n, E, H)
    rc.play(hs, ref, rc.OracleGame(n, E, 4, 3), 20, 7, "checkpoint", every=20)
    other = HostStore(hostlib, n, E, H, B, begin=False)
    other.ws[:] = hs.ws
    rc.check_store(other, ref, "the copy")
    rc.same_batch(other.sample(B, 1, 1, 2, 3), ref.sample(B, 1, 1, 2, 3).arrays(), "the copy's sample")
