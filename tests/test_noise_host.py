"""The root noise's core (csrc/noise.hpp: whether a board takes noise, a square's
table draw, one row's two passes -- the text the device kernel runs on a lane a
board, compiled for the host with g++: tests/host/noise_host.cpp) against the Python
integers of tests/noise_ref.py on every case of tests/noise_cases.py, with guard
words behind the output.  Every comparison is exact equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import noise_cases as nz
import noise_ref as nf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "noise_host.cpp")
LIB = os.path.join(HERE, "host", "libnoise_host.so")
HDRS = [os.path.join(ROOT, "gymothelloenv_amd", "csrc", f) for f in ("noise.hpp", "bitboard.hpp")]
GUARD = 64  # elements behind the output that no call may touch


def load_hostlib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    P, I = ctypes.c_void_p, ctypes.c_int
    L.host_puct_noise.argtypes = [I, I, I, P, P, P, P, P, P, ctypes.c_int32, P, ctypes.c_uint64, ctypes.c_uint32,
                                  ctypes.c_uint64]
    return L


@pytest.fixture(scope="module")
def hostlib():
    return load_hostlib()


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run(L, c, epsilon, inplace):
    """The host build on case c: the output (E K, nn)."""
    count = c.priors.size
    whole = np.full(count + GUARD, 7, dtype=np.int32)
    out = whole[:count].reshape(c.priors.shape)
    src = c.priors.copy()
    if inplace:
        out[:] = src
        src = out
    table = np.ascontiguousarray(c.table, dtype=np.uint32)
    rc = L.host_puct_noise(c.n, nz.E, c.K, ptr(c.handle_boards), ptr(c.handle_legal), ptr(c.kind), ptr(c.boards), ptr(src),
                           ptr(out), epsilon, ptr(table), c.seed, (c.id_key + c.id_base) % 2 ** 32, c.counter)
    assert rc == 0
    assert (whole[count:] == 7).all(), "the call wrote behind its output"
    if not inplace:
        assert (src == c.priors).all(), "the call wrote its input"
    return out.copy()


@pytest.mark.parametrize("key", nz.TABLE_KEYS, ids=nz.TABLE_IDS)
def test_exact_against_the_reference(hostlib, key):
    n, K, mode, inplace = key
    c = nz.make(n, K, mode)
    nn = n * n
    for epsilon in nz.EPSILONS:
        want, applied = nz.expected(c, epsilon)
        nz.check_coverage(c, epsilon, want, applied)
        got = run(hostlib, c, epsilon, inplace)
        np.testing.assert_array_equal(got, want, err_msg="epsilon %d" % epsilon)
        if epsilon == 0:  # the clamped inputs on the legal squares of the applied rows, and nothing else
            clamped = 0
            for e in np.flatnonzero(applied):
                sq = nf.legal_squares(c.handle_legal[e], nn)
                row = c.priors[e * K].copy()
                row[sq] = np.clip(row[sq], 0, 65535)
                if (got[e * K] == c.priors[e * K]).all():
                    continue  # nothing to clamp, or a row whose draws were all zero: copied
                np.testing.assert_array_equal(got[e * K], row)
                clamped += 1
            assert clamped > 10


@pytest.mark.parametrize("i", range(len(nz.SPECIAL)), ids=nz.SPECIAL_IDS)
def test_special_cases(hostlib, i):
    name, kw = nz.SPECIAL[i]
    c = nz.make(**kw)
    for epsilon in (64, 256):
        want, applied = nz.expected(c, epsilon)
        nz.check_coverage(c, epsilon, want, applied)
        for inplace in (False, True):
            np.testing.assert_array_equal(run(hostlib, c, epsilon, inplace), want, err_msg=name)
        if name == "zero-table":
            assert (want == c.priors).all(), "an all-zero table copies every row"
        if name.startswith("clamped"):  # every entry at or above 2^24 counts as 2^24
            capped = c._replace(table=np.minimum(c.table, 1 << 24).astype(np.uint32))
            np.testing.assert_array_equal(nz.expected(capped, epsilon)[0], want)
            assert (want != nz.expected(c._replace(table=(c.table & 0xFFFFFF).astype(np.uint32)), epsilon)[0]).any()


def test_the_id_wraps(hostlib):
    """Board e under id_key = 2^32 - k is board e - k under id_key 0: the draw depends on id_key + env_id_base + e
    mod 2^32 alone."""
    k = 3
    a = nz.make(8, 1, "root")
    roll = lambda x: np.roll(x, k, axis=0)  # noqa: E731  (board e of b is board e - k of a)
    b = a._replace(handle_boards=roll(a.handle_boards), handle_legal=roll(a.handle_legal), priors=roll(a.priors),
                   id_key=2 ** 32 - k)
    out_a, out_b = run(hostlib, a, 64, False), run(hostlib, b, 64, False)
    np.testing.assert_array_equal(out_b[k:], out_a[:-k])
    np.testing.assert_array_equal(out_b, nz.expected(b, 64)[0])
    split = a._replace(id_key=5, id_base=2 ** 32 - 5)  # the two add up to 0 mod 2^32
    np.testing.assert_array_equal(run(hostlib, split, 64, False), out_a)


def test_draws_differ_by_counter_seed_and_board(hostlib):
    c = nz.make(8, 1, "root")
    base = run(hostlib, c, 256, False)
    assert (run(hostlib, c._replace(counter=c.counter + 1), 256, False) != base).any()
    assert (run(hostlib, c._replace(counter=c.counter + 2 ** 32), 256, False) != base).any()
    assert (run(hostlib, c._replace(seed=c.seed ^ 1), 256, False) != base).any()
    assert (run(hostlib, c._replace(seed=c.seed ^ (1 << 63)), 256, False) != base).any()
    # two boards with the same row and the same moves draw differently
    same = c._replace(handle_legal=np.tile(c.handle_legal[2], (nz.E, 1)), priors=np.tile(c.priors[2], (nz.E, 1)))
    out = run(hostlib, same, 256, False)
    assert len(set(map(bytes, out))) == nz.E
    # epsilon = 256 on every square: the row is eta alone and sums to 65535 within the rounding
    assert (np.abs(out.sum(1) - 65535) <= 64).all()


def test_refusals(hostlib):
    c = nz.make(8, 1, "leaf")
    out = np.full_like(c.priors, 7)
    t = np.ascontiguousarray(c.table)
    args = [8, nz.E, 1, ptr(c.handle_boards), ptr(c.handle_legal), ptr(c.kind), ptr(c.boards), ptr(c.priors), ptr(out), 64,
            ptr(t), 1, 0, 0]
    for at, bad in ((5, None), (6, None), (9, -1), (9, 257), (2, 0), (2, 65), (0, 3), (0, 17), (10, None)):
        a = list(args)
        a[at] = bad
        assert hostlib.host_puct_noise(*a) == 1
    assert (out == 7).all()
