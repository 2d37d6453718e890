"""OneWord<N>::flip_fills (csrc/bitboard.hpp: update_board's flips from the legal
scan's fills and four ray constants shifted to the square, no ray table and no
edge masks -- the play kernels' flips) compiled for the host with g++, against
the oracle's cell-by-cell update_board on every empty square of random boards
and of positions from random games, N = 4..8; and the same source as a
stand-alone program under -fsanitize=undefined over a = -2..66."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "flip_rays_host.cpp")
LIB = os.path.join(HERE, "host", "libflip_rays_host.so")
HDR = os.path.join(os.path.dirname(HERE), "gymothelloenv_amd", "csrc", "bitboard.hpp")


@pytest.fixture(scope="module")
def hostlib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    P = ctypes.c_void_p
    L.host_flip_fills_all.argtypes = [ctypes.c_int, ctypes.c_int, P, P, ctypes.c_int, P, P]
    return L


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def random_boards(n, E, rng, density):
    cells = rng.choice(3, size=(E, n * n), p=[1 - density, density / 2, density / 2])
    mover = np.zeros(E, dtype=np.uint64)
    opp = np.zeros(E, dtype=np.uint64)
    for a in range(n * n):
        mover |= (cells[:, a] == 1).astype(np.uint64) << np.uint64(a)
        opp |= (cells[:, a] == 2).astype(np.uint64) << np.uint64(a)
    return mover, opp


def game_positions(n, E, seed):
    """(mover, opp) of E boards after every ply of two games' worth of random play
    by the bitboard CPU engine from the standard opening (auto-reset in between)."""
    movers, opps = [], []
    s = oracle.reset(n, E)
    for k in range(2 * (n * n - 4)):  # two games' worth of plies, auto-reset in between
        oracle.bb_rollout(s, 1, seed=seed, ply0=k, record=False)
        tw = (s.meta & 1) != 0
        movers.append(np.where(tw, s.boards[:, 1], s.boards[:, 0]))
        opps.append(np.where(tw, s.boards[:, 0], s.boards[:, 1]))
    return np.concatenate(movers), np.concatenate(opps)


def oracle_flips(n, mover, opp):
    """update_board's flips from every square: [E, n*n] (the mover plays white)."""
    E = len(mover)
    out = np.zeros((E, n * n), dtype=np.uint64)
    for a in range(n * n):
        s = oracle.State(n, E)
        s.boards[:, 0] = opp
        s.boards[:, 1] = mover
        s.meta[:] = oracle.meta_from(np.ones(E))
        oracle.update_board(s, np.full(E, a, dtype=np.int32))
        out[:, a] = opp & ~s.boards[:, 0]
    return out


@pytest.fixture(scope="module", params=[4, 5, 6, 7, 8])
def sample(request):
    """The boards of one size and the oracle's flips from each of their squares, computed once."""
    n = request.param
    rng = np.random.RandomState(700 + n)
    parts = [random_boards(n, 1200, rng, d) for d in (0.3, 0.6, 0.8, 0.95)]
    parts.append(game_positions(n, 24, seed=n))
    mover = np.ascontiguousarray(np.concatenate([p[0] for p in parts]))
    opp = np.ascontiguousarray(np.concatenate([p[1] for p in parts]))
    return n, mover, opp, oracle_flips(n, mover, opp)


@pytest.mark.parametrize("scan", [0, 1], ids=["legal_moves_fills", "OneWord_legal"])
def test_flip_fills_every_empty_square(hostlib, sample, scan):
    n, mover, opp, want = sample
    E, nn = len(mover), n * n
    legal = np.zeros(E, dtype=np.uint64)
    got = np.zeros((E, nn), dtype=np.uint64)
    assert hostlib.host_flip_fills_all(n, E, ptr(mover), ptr(opp), scan, ptr(legal), ptr(got)) == 0
    a = np.arange(nn, dtype=np.uint64)
    empty = (((mover | opp)[:, None] >> a) & np.uint64(1)) == 0
    np.testing.assert_array_equal(got, np.where(empty, want, np.uint64(0)))
    # a move flips something exactly on the legal squares
    moves = empty & (want != 0)
    np.testing.assert_array_equal(moves, ((legal[:, None] >> a) & np.uint64(1)) == 1)
    # the sample plays where an unmasked ray wraps: all four corners and both edge columns
    played = moves.any(axis=0)
    corners = [0, n - 1, nn - n, nn - 1]
    assert all(played[c] for c in corners), (n, [c for c in corners if not played[c]])
    for col in (0, n - 1):
        assert any(played[r * n + col] for r in range(1, n - 1)), (n, col)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_flip_fills_shift_counts_under_ubsan(tmp_path):
    """Every a in [-2, 66] (invalid actions included: the callers mask their flips)
    keeps every shift count defined."""
    exe = str(tmp_path / "flip_rays_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
                           "-DFLIP_RAYS_MAIN", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           "-static-libubsan", "-o", exe, SRC])
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "clean" in r.stdout
