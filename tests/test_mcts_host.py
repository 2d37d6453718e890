"""The tree search's core (csrc/mcts.hpp, the text the device kernel runs,
compiled for the host with g++: tests/host/mcts_host.cpp) against the plain
Python integers of tests/mcts_ref.py.  Every comparison is exact equality."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import family_cases as fc
import mcts_ref as mr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "mcts_host.cpp")
LIB = os.path.join(HERE, "host", "libmcts_host.so")
HDRS = [os.path.join(ROOT, "gymothelloenv_amd", "csrc", f) for f in ("mcts.hpp", "root_tasks.hpp", "bitboard.hpp")]


@pytest.fixture(scope="module")
def hostlib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    P = ctypes.c_void_p
    L.host_mcts.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
                            ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, P, P, P, P,
                            P]
    L.host_mcts_isqrt.argtypes = [ctypes.c_uint64]
    L.host_mcts_isqrt.restype = ctypes.c_uint32
    return L


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_mcts(L, s, I, R, C, T, seed=mr.SEED, id_key=mr.ID_KEY, id_base=mr.ID_BASE, counter=mr.COUNTER):
    nn = s.n * s.n
    visits, wins2 = np.full((s.E, nn), 7, dtype=np.int32), np.full((s.E, nn), 7, dtype=np.int32)
    best, nodes = np.full(s.E, 7, dtype=np.int32), np.full(s.E, 7, dtype=np.int32)
    status = np.full(s.E, 7, dtype=np.uint8)
    assert L.host_mcts(s.n, s.E, ptr(s.boards), ptr(s.meta), ptr(s.legal), id_base, I, R, C, T, seed, id_key, counter,
                       ptr(visits), ptr(wins2), ptr(best), ptr(nodes), ptr(status)) == 0
    return visits, wins2, best, nodes, status


NAMES = ("visits", "wins2", "best", "tree_nodes", "status")


@pytest.mark.parametrize("c", mr.CASES, ids=lambda c: "n%d-E%d-I%d-R%d-C%d-T%d" % c)
def test_exact_against_the_reference(hostlib, c):
    s, res = mr.case(c)
    mr.check_case(c, res)
    n, E, I, R, C, T = c
    for name, g, w in zip(NAMES, host_mcts(hostlib, s, I, R, C, T), res.outputs()):
        np.testing.assert_array_equal(g, w, err_msg=name)


def test_isqrt(hostlib):
    xs = [0, 1, 2 ** 32 - 1]
    for k in range(1, 65536):
        xs += [k * k - 1, k * k, k * k + 1]
    for x in xs:
        assert hostlib.host_mcts_isqrt(x) == math.isqrt(x), x


def test_key_and_seed_matter(hostlib):
    c = mr.CASES[1]
    s, res = mr.case(c)
    n, E, I, R, C, T = c
    same = host_mcts(hostlib, s, I, R, C, T)
    np.testing.assert_array_equal(same[1], res.wins2)
    for kw in (dict(seed=mr.SEED + 1), dict(id_key=mr.ID_KEY + 1), dict(counter=mr.COUNTER + 1),
               dict(id_base=mr.ID_BASE + 1)):
        assert (host_mcts(hostlib, s, I, R, C, T, **kw)[1] != res.wins2).any(), kw


@pytest.mark.parametrize("c", [fc.mcts_case(n) for n in fc.NEW_SIZES] + [fc.mcts_case(n, full=True) for n in fc.MCTS_FULL],
                         ids=lambda c: "n%d-E%d-I%d-R%d-C%d-T%d" % c)
def test_every_other_size_against_the_reference(hostlib, c):
    """The board sizes mcts_ref.CASES leaves out: the device's cases of tests/test_gpu_family_sizes.py on the host build."""
    assert sorted({k[0] for k in mr.CASES} | set(fc.NEW_SIZES)) == fc.ALL_SIZES
    test_exact_against_the_reference(hostlib, c)
