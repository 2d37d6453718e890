"""The play-search core (csrc/play_search.hpp's shared part over csrc/search.hpp,
the text the device kernel runs, compiled for the host with g++:
tests/host/play_search_host.cpp) against the reference of the searched move in
tests/play_search_ref.py; SearchConfig's validation and the C ABI's bindings.
Every comparison is exact equality."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import family_cases as fc
import play_search_ref as pr
import search_ref as sh
import solve_ref as sr
from oracle import oracle
from test_search_host import searchlib  # noqa: F401  (the fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "play_search_host.cpp")
LIB = os.path.join(HERE, "host", "libplay_search_host.so")
HDRS = [os.path.join(ROOT, "gymothelloenv_amd", "csrc", f)
        for f in ("play_search.hpp", "search.hpp", "root_tasks.hpp", "bitboard.hpp")]
SIZES = [4, 5, 6, 8, 10, 16]


@pytest.fixture(scope="module")
def movelib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    P = ctypes.c_void_p
    L.host_search_move.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_uint64, P, P]
    return L


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_search_move(L, s, cfg):
    w = np.ascontiguousarray(cfg.weights, dtype=np.int8)
    assert w.shape == (s.n * s.n,)
    act, fb = np.full(s.E, 7, dtype=np.int32), np.full(s.E, 7, dtype=np.uint8)
    assert L.host_search_move(s.n, s.E, ptr(s.boards), ptr(s.meta), ptr(s.legal), cfg.depth, ptr(w), cfg.mobility,
                              cfg.terminal, cfg.endgame_empties, cfg.max_nodes, ptr(act), ptr(fb)) == 0
    return act, fb


def cases(n):
    """(state, black's policy, white's policy) of a size: the self-play case's
    policies on the search batch.  At n = 4 a second batch (seed 2) comes with it:
    few 4x4 searches place 40 discs under one root move, and one batch holds 3
    fallbacks of black's policy where the test wants 5."""
    s, _ = sh.batch(n, 74)
    if n == 4:
        s = sr.join(s, sh.batch(n, 74, seed=2)[0])
    return s, pr.black_policy(n), pr.white_policy(n)


@pytest.mark.parametrize("n", SIZES)
def test_greedy_equivalent_policy(searchlib, n):  # noqa: F811
    """GEQ's searched move is oracle.greedy's on every live board, by the reference alone."""
    s, _ = sh.batch(n, 74)
    act, fb, _ = pr.searched_moves(searchlib, s, pr.geq(n), pr.geq(n))
    live = (s.meta & 2) == 0
    assert live.sum() > 50 and not fb.any()
    np.testing.assert_array_equal(act[live], oracle.greedy(s)[live])


@pytest.mark.parametrize("n", SIZES)
def test_equals_the_reference(searchlib, movelib, n):  # noqa: F811
    s, black, white = cases(n)
    got_b, got_w = host_search_move(movelib, s, black), host_search_move(movelib, s, white)
    # each policy over the whole batch, whoever is to move
    for cfg, got in ((black, got_b), (white, got_w)):
        a, f, end = pr.searched_moves(searchlib, s, cfg, cfg)
        if cfg is black:  # by the reference alone: the batch holds fallbacks and endgame-mode boards
            assert f.sum() >= 5 and end.sum() >= 5, (int(f.sum()), int(end.sum()))
        assert (a[[0, 2]] == -1).all() and not f[[0, 2]].any()  # the terminated board and the empty mask
        np.testing.assert_array_equal(got[0], a)
        np.testing.assert_array_equal(got[1], f)
    # and each board by its mover's policy, as self-play picks it
    tw = (s.meta & 1) != 0
    a, f, _ = pr.searched_moves(searchlib, s, black, white)
    np.testing.assert_array_equal(np.where(tw, got_w[0], got_b[0]), a)
    np.testing.assert_array_equal(np.where(tw, got_w[1], got_b[1]), f)


def test_argument_refusals(movelib):
    s, _ = sh.batch(4, 74)
    w = np.ones(16, dtype=np.int8)
    out = [np.zeros(s.E, dtype=np.int32), np.zeros(s.E, dtype=np.uint8)]
    for depth, mob, term, end, budget in ((0, 0, 64, 0, 1), (15, 0, 64, 0, 1), (1, 128, 64, 0, 1), (1, -128, 64, 0, 1),
                                          (1, 0, 0, 0, 1), (1, 0, 32768, 0, 1), (1, 0, 64, -1, 1), (1, 0, 64, 15, 1),
                                          (1, 0, 64, 0, 0), (1, 0, 64, 0, 1 << 32)):
        assert movelib.host_search_move(s.n, s.E, ptr(s.boards), ptr(s.meta), ptr(s.legal), depth, ptr(w), mob, term,
                                        end, budget, ptr(out[0]), ptr(out[1])) == -1


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_play_search_core_under_asan_ubsan(searchlib, tmp_path):  # noqa: F811
    """A stand-alone program (its own main, nothing loaded into Python) runs the
    host core over the same inputs: one-, two- and four-word boards, both policies."""
    lines = []
    for n in SIZES:
        s, black, white = cases(n)
        for cfg in (black, white):
            act, fb, _ = pr.searched_moves(searchlib, s, cfg, cfg)
            for e in range(s.E):
                words = list(s.boards[e]) + list(s.legal[e])
                lines.append("%d %d %d %d %d %d %d %d %d %s %s" % (
                    n, s.meta[e], cfg.depth, cfg.mobility, cfg.terminal, cfg.endgame_empties, cfg.max_nodes, act[e],
                    fb[e], " ".join("%x" % int(x) for x in words), " ".join("%d" % int(x) for x in cfg.weights)))
    pos = tmp_path / "positions.txt"
    pos.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "play_search_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DPLAY_SEARCH_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(pos)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d positions clean" % len(lines) in r.stdout


def test_search_config_validation():
    import torch
    from gymothelloenv_amd import SearchConfig, policies
    assert policies.SearchConfig is SearchConfig
    c = SearchConfig()
    assert (c.depth, c.weights, c.mobility, c.terminal, c.endgame_empties, c.max_nodes) == (4, None, 0, 64, 0, 1 << 22)
    c = SearchConfig(depth=14, weights=np.arange(64) - 32, mobility=-127, terminal=32767, endgame_empties=14,
                     max_nodes=2 ** 32 - 1)
    assert c.weights.dtype == torch.int8 and c.weights.numel() == 64
    assert SearchConfig(weights=torch.zeros(10, 10, dtype=torch.int64)).weights.shape == (10, 10)
    for bad in (dict(depth=0), dict(depth=15), dict(mobility=128), dict(mobility=-128), dict(terminal=0),
                dict(terminal=32768), dict(endgame_empties=-1), dict(endgame_empties=15), dict(max_nodes=0),
                dict(max_nodes=2 ** 32), dict(depth=2.5), dict(weights=np.full(64, 128)),
                dict(weights=np.zeros(63, dtype=np.int8)), dict(weights=np.zeros(64, dtype=np.float32)),
                dict(weights=np.zeros((8, 9), dtype=np.int8))):
        with pytest.raises(ValueError):
            SearchConfig(**bad)


def test_signatures_and_struct():
    """The three entry points are bound with the header's argument lists, and the
    struct has the header's layout."""
    from gymothelloenv_amd import _lib as L
    P, I32 = ctypes.c_void_p, ctypes.c_int32
    assert L.SIGNATURES["oth_play_search"] == (I32, [P, P, P, I32, P, P, P, P, P])
    assert L.SIGNATURES["oth_reset_vs_search"] == (I32, [P, P, P, P, P])
    assert L.SIGNATURES["oth_step_vs_search"] == (I32, [P, P, P, P, P, P, P, P, P])
    S = L.OthSearchPolicy
    assert [(f, getattr(S, f).offset) for f, _ in S._fields_] == [
        ("weights", 0), ("depth", 8), ("mobility_weight", 12), ("terminal_weight", 16), ("endgame_empties", 20),
        ("max_nodes", 24)] and ctypes.sizeof(S) == 32
    header = open(os.path.join(ROOT, "include", "othello_mi355x.h")).read()
    body = header[header.index("typedef struct oth_search_policy {"):header.index("} oth_search_policy;")]
    assert [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.splitlines()[1:] if ";" in ln] == \
        [f for f, _ in S._fields_]


@pytest.mark.parametrize("n", fc.NEW_SIZES_SOLVE)
def test_every_other_size_equals_the_reference(searchlib, movelib, n):  # noqa: F811
    """test_equals_the_reference at the board sizes SIZES leaves out."""
    assert sorted(SIZES + fc.NEW_SIZES_SOLVE) == fc.ALL_SIZES
    test_equals_the_reference(searchlib, movelib, n)
