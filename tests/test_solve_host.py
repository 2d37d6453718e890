"""The solver's search core (csrc/solve.hpp, the text the device kernel runs,
compiled for the host with g++: tests/host/solve_host.cpp) against the plain
minimax of tests/solve_ref.py.  Every comparison is exact equality."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import family_cases as fc
import solve_ref as sr
from oracle import oracle
from test_bitboard_host import random_boards

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "solve_host.cpp")
LIB = os.path.join(HERE, "host", "libsolve_host.so")
HDRS = [os.path.join(ROOT, "gymothelloenv_amd", "csrc", f) for f in ("solve.hpp", "root_tasks.hpp", "bitboard.hpp")]
BIG = 1 << 24  # a budget no test position reaches


@pytest.fixture(scope="module")
def hostlib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    P = ctypes.c_void_p
    L.host_solve.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, ctypes.c_int, ctypes.c_uint64, P, P, P, P, P]
    L.host_solve_flips_all.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P]
    return L


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_solve(L, s, max_empties=sr.MAX_EMPTIES, max_nodes=BIG):
    nn = s.n * s.n
    value, best = np.full(s.E, 7, dtype=np.int32), np.full(s.E, 7, dtype=np.int32)
    mv = np.full((s.E, nn), 7, dtype=np.int32)
    status, nodes = np.full(s.E, 7, dtype=np.uint8), np.full(s.E, 7, dtype=np.uint64)
    assert L.host_solve(s.n, s.E, ptr(s.boards), ptr(s.meta), ptr(s.legal), max_empties, max_nodes, ptr(value),
                        ptr(best), ptr(mv), ptr(status), ptr(nodes)) == 0
    return value, best, mv, status, nodes


def assert_equals_reference(got, res):
    for name, g, w in zip(("value", "best", "move_values", "status"), got, res.outputs()):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert (got[4] <= res.nodes).all()
    assert (got[4][res.status != sr.EXACT] == 0).all() and (got[4][res.status == sr.EXACT] > 0).all()


@pytest.mark.parametrize("n", [4, 5, 6, 7, 8])
def test_flips_from_the_discs_alone(hostlib, n):
    """solve_flips1 of every empty square: the oracle's update_board on the legal
    ones, nothing on the others."""
    rng = np.random.RandomState(70 + n)
    nn = n * n
    for density in (0.5, 0.8, 0.95):
        _, mover, opp = random_boards(n, 400, rng, density)
        E = len(mover)
        out = np.zeros((E, nn), dtype=np.uint64)
        assert hostlib.host_solve_flips_all(n, E, ptr(mover), ptr(opp), ptr(out)) == 0
        lb = sr.legal_rows(oracle.legal(n, mover, opp), nn)
        np.testing.assert_array_equal(out != 0, lb)
        for a in range(nn):
            at = np.flatnonzero(lb[:, a])
            if not len(at):
                continue
            s = oracle.State(n, len(at))
            s.boards[:] = np.concatenate([mover[at], opp[at]], axis=1)  # black = the mover
            oracle.update_board(s, np.full(len(at), a, dtype=np.int32))
            np.testing.assert_array_equal(out[at, a], opp[at, 0] & ~s.boards[:, 1])


def test_the_whole_4x4_game(hostlib):
    s = oracle.reset(4, 1)
    res = sr.solve(s)
    assert res.value[0] == -8 and res.nodes[0] > 190000  # black, to move, loses by eight
    got = host_solve(hostlib, s, max_empties=12)
    assert got[0][0] == -8
    assert_equals_reference(got, res)
    assert host_solve(hostlib, s, max_empties=11)[3][0] == sr.SKIPPED
    # every position of one random 4x4 game
    game = oracle.State(4, 13)
    one = oracle.reset(4, 1)
    for p in range(13):
        sr.put(game, p, one)
        if not int(one.meta[0]) & 2:
            oracle.rollout(one, 0, 0, 1, seed=5, id_base=3, ply0=p, record=False)
    assert int(game.meta[-1]) & 2 and not int(game.meta[5]) & 2
    assert_equals_reference(host_solve(hostlib, game), sr.solve(game))


@pytest.mark.parametrize("n,max_e", [(4, 9), (5, 9), (6, 9), (8, 9), (10, 7), (16, 5)])
def test_exact_against_the_reference(hostlib, n, max_e):
    s, res, full = sr.batch(n, 37, max_e)
    sr.check_batch(s, res, full)  # the specials are in the batch
    assert_equals_reference(host_solve(hostlib, s), res)
    cut = max_e - 3  # some boards are SKIPPED
    res_cut = sr.solve(s, max_empties=cut)
    assert (res_cut.status == sr.SKIPPED).any() and (res_cut.status == sr.EXACT).any()
    assert_equals_reference(host_solve(hostlib, s, max_empties=cut), res_cut)


def test_pruning_happens(hostlib):
    s = sr.late_positions(8, 12, [8, 9], seed=11)
    res = sr.solve(s)
    assert (res.status == sr.EXACT).all() and (8 * 8 - oracle.count_disks(s).sum(1) >= 8).all()
    got = host_solve(hostlib, s)
    assert_equals_reference(got, res)
    assert int(got[4].sum()) < int(res.nodes.sum())


def test_budget(hostlib):
    s, res, _ = sr.batch(8, 37, 9)
    nn = 64
    counts = sr.legal_rows(s.legal, nn).sum(1)
    seen = 0
    for e in np.flatnonzero((res.status == sr.EXACT) & (counts >= 3)):
        squares = np.flatnonzero(sr.legal_rows(s.legal[e:e + 1], nn)[0])
        one = sr.subset(s, [e] * len(squares))  # the board narrowed to each of its root moves
        for k, a in enumerate(squares):
            one.legal[k] = sr.mask_words([a], 8)
        v, b, mv, st, per = host_solve(hostlib, one)
        assert (st == sr.EXACT).all() and (b == squares).all()
        np.testing.assert_array_equal(v, res.move_values[e, squares])
        big = int(np.argmax(per))
        if per[big] < 2 or (per == per[big]).sum() != 1:
            continue
        seen += 1
        k1 = sr.subset(one, [big])
        for budget, want in ((int(per[big]), sr.EXACT), (int(per[big]) - 1, sr.ABORTED)):
            v1, b1, mv1, st1, nd1 = host_solve(hostlib, k1, max_nodes=budget)
            assert st1[0] == want
            if want == sr.EXACT:
                assert v1[0] == v[big] and b1[0] == squares[big] and nd1[0] == per[big]
            else:
                assert v1[0] == sr.NO_VALUE and b1[0] == -1 and (mv1 == sr.NO_VALUE).all() and nd1[0] == per[big]
        # the whole board with only its largest task over budget: the finished moves keep their values
        budget = int(per[big]) - 1
        assert (np.delete(per, big) <= budget).all()
        v2, b2, mv2, st2, nd2 = host_solve(hostlib, sr.subset(s, [e]), max_nodes=budget)
        assert st2[0] == sr.ABORTED and v2[0] == sr.NO_VALUE and b2[0] == -1
        want_mv = res.move_values[e].copy()
        want_mv[squares[big]] = sr.NO_VALUE
        np.testing.assert_array_equal(mv2[0], want_mv)
        assert (want_mv != sr.NO_VALUE).sum() == len(squares) - 1
        assert nd2[0] == per.sum()  # the abandoned move adds budget + 1, its own count here
    assert seen >= 3


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_search_core_under_asan_ubsan(tmp_path):
    """A stand-alone program (its own main, nothing loaded into Python) runs the
    host core over the golden file's positions."""
    from test_solve_golden import golden_states
    lines = []
    for s, value, best, _, _ in golden_states():
        for e in range(s.E):
            words = list(s.boards[e]) + list(s.legal[e])
            lines.append("%d %d %d %d %s" % (s.n, s.meta[e], value[e], best[e], " ".join("%x" % int(w) for w in words)))
    # two-word and four-word frames as well: positions valued by the reference here
    for n, max_e in ((10, 4), (16, 3)):
        s = sr.late_positions(n, 6, list(range(1, max_e + 1)), seed=3)
        res = sr.solve(s)
        for e in np.flatnonzero(res.status == sr.EXACT):
            words = list(s.boards[e]) + list(s.legal[e])
            lines.append("%d %d %d %d %s" % (n, s.meta[e], res.value[e], res.best[e],
                                             " ".join("%x" % int(w) for w in words)))
    pos = tmp_path / "positions.txt"
    pos.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "solve_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DSOLVE_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(pos)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d positions clean" % len(lines) in r.stdout


@pytest.mark.parametrize("n", fc.NEW_SIZES_SOLVE)
def test_every_other_size_against_the_reference(hostlib, n):
    """One batch at each board size that the cases above leave out (N = 12 and 13 take three words, 14 and 15 four with
    a partly used last word, 7, 9 and 11 are odd): with them the host build stands in for `nodes` at all 13 sizes."""
    s, res, full = sr.batch(n, 37, fc.solve_max_e(n))
    sr.check_batch(s, res, full)  # the specials are in the batch
    assert_equals_reference(host_solve(hostlib, s), res)
