"""The search core (csrc/search.hpp, the text the device kernel runs, compiled
for the host with g++: tests/host/search_host.cpp) against the plain minimax
of tests/search_ref.py.  Every comparison is exact equality."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import family_cases as fc
import search_ref as sh
import solve_ref as sr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "search_host.cpp")
LIB = os.path.join(HERE, "host", "libsearch_host.so")
HDRS = [os.path.join(ROOT, "gymothelloenv_amd", "csrc", f) for f in ("search.hpp", "root_tasks.hpp", "bitboard.hpp")]
BIG = 1 << 24  # a budget no test position reaches
SIZES = [4, 5, 6, 8, 10, 16]
WSETS = ["default", "random", "ones"]


@pytest.fixture(scope="module")
def searchlib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    P = ctypes.c_void_p
    L.host_search.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int,
                              ctypes.c_uint64, P, P, P, P, P]
    return L


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_search(L, s, depth, weights, mobility=0, terminal=64, max_nodes=BIG):
    nn = s.n * s.n
    w = np.ascontiguousarray(weights, dtype=np.int8)
    assert w.shape == (nn,)
    value, best = np.full(s.E, 7, dtype=np.int32), np.full(s.E, 7, dtype=np.int32)
    mv = np.full((s.E, nn), 7, dtype=np.int32)
    status, nodes = np.full(s.E, 7, dtype=np.uint8), np.full(s.E, 7, dtype=np.uint64)
    assert L.host_search(s.n, s.E, ptr(s.boards), ptr(s.meta), ptr(s.legal), depth, ptr(w), mobility, terminal,
                         max_nodes, ptr(value), ptr(best), ptr(mv), ptr(status), ptr(nodes)) == 0
    return value, best, mv, status, nodes


def assert_equals_reference(got, res):
    for name, g, w in zip(("value", "best", "move_values", "status"), got, res.outputs()):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert (got[4] <= res.nodes).all()
    assert (got[4][res.status != sh.DONE] == 0).all() and (got[4][res.status == sh.DONE] > 0).all()


def test_default_weights():
    from gymothelloenv_amd import default_search_weights
    for n in range(4, 17):
        w = default_search_weights(n)
        assert tuple(w.shape) == (n, n) and str(w.dtype) == "torch.int8"
        np.testing.assert_array_equal(w.numpy().reshape(-1), sh.default_weights(n))
    w8 = default_search_weights(8).numpy()
    assert w8[0].tolist() == [100, -20, 10, 10, 10, 10, -20, 100] and w8[1].tolist() == [-20, -50, 0, 0, 0, 0, -50, -20]
    assert default_search_weights(4).numpy().tolist() == [[100, -20, -20, 100], [-20, -50, -50, -20],
                                                          [-20, -50, -50, -20], [100, -20, -20, 100]]


@pytest.mark.parametrize("wname", WSETS)
@pytest.mark.parametrize("n", SIZES)
def test_equals_the_reference(searchlib, n, wname):
    for depth in sh.depths(n):
        s, res, (w, mob, term) = sh.reference(n, 74, depth, wname)
        got = host_search(searchlib, s, depth, w, mob, term)
        assert_equals_reference(got, res)
        assert (res.status == sh.DONE).sum() > 30


def test_pruning_happens(searchlib):
    s, res, (w, mob, term) = sh.reference(8, 74, 4, "default")
    got = host_search(searchlib, s, 4, w, mob, term)
    assert int(got[4].sum()) < int(res.nodes.sum()) // 2


def test_positive_mobility(searchlib):
    """The three sets carry mobility 0 (the frontier's second scan skipped where the
    first is non-empty) and -127; here small positive ones over the same boards."""
    for n, mob in ((8, 1), (10, 127)):
        s, _, (w, _, term) = sh.reference(n, 74, 2, "ones")
        res = sh.search(s, 2, w, mob, term)
        assert_equals_reference(host_search(searchlib, s, 2, w, mob, term), res)


@pytest.mark.parametrize("n,max_e", [(4, 9), (8, 9), (10, 7), (16, 5)])
def test_depth_beyond_the_end_is_the_solver(searchlib, n, max_e):
    """No leaf is heuristic: with terminal 1 the values are oth_solve's, whatever the weights."""
    s, res, _ = sr.batch(n, 37, max_e)
    w = sh.weight_sets(n)["random"][0]
    value, best, mv, status, nodes = host_search(searchlib, s, 14, w, -127, 1)
    np.testing.assert_array_equal(status, res.status)  # (EXACT is DONE; no board is SKIPPED at 14)
    live = res.status == sr.EXACT
    assert live.sum() > 20
    np.testing.assert_array_equal(value[live], res.value[live])
    np.testing.assert_array_equal(value[res.status == sr.TERMINATED], res.value[res.status == sr.TERMINATED])
    np.testing.assert_array_equal(best, res.best)
    np.testing.assert_array_equal(mv, np.where(res.move_values == sr.NO_VALUE, sh.NO_VALUE, res.move_values))


def budget_cases(run, depth=3, wname="default"):
    """The budget cases on run(state, max_nodes=...) -> the five outputs: shared with the device's test."""
    s, res, _ = sh.reference(8, 74, depth, wname)
    counts = sr.legal_rows(s.legal, 64).sum(1)
    seen = 0
    for e in np.flatnonzero((res.status == sh.DONE) & (counts >= 3)):
        squares = np.flatnonzero(sr.legal_rows(s.legal[e:e + 1], 64)[0])
        one = sr.subset(s, [e] * len(squares))  # the board narrowed to each of its root moves
        for k, a in enumerate(squares):
            one.legal[k] = sr.mask_words([a], 8)
        v, b, mv, st, per = run(one)
        assert (st == sh.DONE).all() and (b == squares).all()
        np.testing.assert_array_equal(v, res.move_values[e, squares])
        big = int(np.argmax(per))
        if per[big] < 2 or (per == per[big]).sum() != 1:
            continue
        seen += 1
        k1 = sr.subset(one, [big])
        for budget, want in ((int(per[big]), sh.DONE), (int(per[big]) - 1, sh.ABORTED)):
            v1, b1, mv1, st1, nd1 = run(k1, max_nodes=budget)
            assert st1[0] == want
            if want == sh.DONE:
                assert v1[0] == v[big] and b1[0] == squares[big] and nd1[0] == per[big]
            else:
                assert v1[0] == sh.NO_VALUE and b1[0] == -1 and (mv1 == sh.NO_VALUE).all() and nd1[0] == per[big]
        # the whole board with only its largest task over budget: the finished moves keep their values
        budget = int(per[big]) - 1
        assert (np.delete(per, big) <= budget).all()
        v2, b2, mv2, st2, nd2 = run(sr.subset(s, [e]), max_nodes=budget)
        assert st2[0] == sh.ABORTED and v2[0] == sh.NO_VALUE and b2[0] == -1
        want_mv = res.move_values[e].copy()
        want_mv[squares[big]] = sh.NO_VALUE
        np.testing.assert_array_equal(mv2[0], want_mv)
        assert (want_mv != sh.NO_VALUE).sum() == len(squares) - 1
        assert nd2[0] == per.sum()  # the abandoned move adds budget + 1, its own count here
        if seen == 3:
            break
    assert seen == 3


def test_budget(searchlib):
    _, _, (w, mob, term) = sh.reference(8, 74, 3, "default")
    budget_cases(lambda st, max_nodes=BIG: host_search(searchlib, st, 3, w, mob, term, max_nodes=max_nodes))


def test_argument_refusals(searchlib):
    s, _, (w, mob, term) = sh.reference(4, 74, 1, "default")
    args = [s.n, s.E, ptr(s.boards), ptr(s.meta), ptr(s.legal)]
    out = [np.zeros(s.E * 16, dtype=np.uint64) for _ in range(5)]
    for depth, mobility, terminal, budget in ((0, 0, 64, 1), (15, 0, 64, 1), (1, 128, 64, 1), (1, -128, 64, 1),
                                              (1, 0, 0, 1), (1, 0, 32768, 1), (1, 0, 64, 0), (1, 0, 64, 1 << 32)):
        assert searchlib.host_search(*(args + [depth, ptr(w), mobility, terminal, budget] + [ptr(o) for o in out])) == -1


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_search_core_under_asan_ubsan(tmp_path):
    """A stand-alone program (its own main, nothing loaded into Python) runs the
    host core over reference positions with one-, two- and four-word boards."""
    lines = []
    for n, depth, wname in ((4, 4, "random"), (6, 3, "default"), (8, 3, "random"), (8, 2, "ones"), (10, 3, "random"),
                            (16, 2, "random"), (16, 3, "default")):
        s, res, (w, mob, term) = sh.reference(n, 74, depth, wname)
        for e in np.flatnonzero(res.status != sh.NO_MOVE)[:40]:
            words = list(s.boards[e]) + list(s.legal[e])
            lines.append("%d %d %d %d %d %d %d %s %s" % (n, s.meta[e], depth, mob, term, res.value[e], res.best[e],
                                                        " ".join("%x" % int(x) for x in words),
                                                        " ".join("%d" % int(x) for x in w)))
    # depth beyond the end: the deepest stacks
    s, res, _ = sr.batch(8, 37, 9)
    w = sh.weight_sets(8)["random"][0]
    for e in np.flatnonzero(res.status == sr.EXACT):
        words = list(s.boards[e]) + list(s.legal[e])
        lines.append("8 %d 14 -127 1 %d %d %s %s" % (s.meta[e], res.value[e], res.best[e],
                                                    " ".join("%x" % int(x) for x in words),
                                                    " ".join("%d" % int(x) for x in w)))
    pos = tmp_path / "positions.txt"
    pos.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "search_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DSEARCH_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(pos)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d positions clean" % len(lines) in r.stdout


@pytest.mark.parametrize("n", fc.NEW_SIZES_SOLVE)
def test_every_other_size_equals_the_reference(searchlib, n):
    """The board sizes SIZES leaves out, one weight set (mobility != 0), depths 1 to 3: with them the host build stands
    in for `nodes` and for the searched moves at all 13 sizes."""
    assert sorted(SIZES + fc.NEW_SIZES_SOLVE) == fc.ALL_SIZES
    for depth in fc.SEARCH_DEPTHS:
        s, res, (w, mob, term) = sh.reference(n, 74, depth, fc.SEARCH_WSET)
        assert mob != 0
        assert_equals_reference(host_search(searchlib, s, depth, w, mob, term), res)
        assert (res.status == sh.DONE).sum() > 30
