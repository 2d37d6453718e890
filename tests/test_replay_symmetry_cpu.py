"""The eight board symmetries of the replay store, on tests/replay_ref.py and on the
host build of csrc/replay.hpp, for every board size: they are eight distinct
permutations of the squares, closed under composition, and legal moves commute
with them -- legal_moves(transformed position) = transformed(legal_moves) --
which is what makes the augmentation of a sample sound."""
import numpy as np
import pytest

import replay_ref as rr
from oracle import oracle
from test_replay_host import hostlib, ptr  # noqa: F401  (the fixture)

SIZES = list(range(4, 17))


def host_perms(L, n):
    return np.array([[L.host_replay_sigma(n, s, a) for a in range(n * n)] for s in range(8)], dtype=np.int64)


def host_masks(L, n, sym, arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint64)
    sym = np.ascontiguousarray(sym, dtype=np.uint8)
    out = np.full_like(arr, 7)
    assert L.host_symmetry_masks(n, arr.shape[0], arr.shape[1], ptr(sym), ptr(arr), ptr(out)) == 0
    return out


@pytest.mark.parametrize("n", SIZES)
def test_eight_distinct_permutations_closed_under_composition(hostlib, n):  # noqa: F811
    p = rr.permutations(n)
    np.testing.assert_array_equal(host_perms(hostlib, n), p)
    assert len({tuple(row) for row in p.tolist()}) == 8
    for s in range(8):
        assert sorted(p[s].tolist()) == list(range(n * n))
    assert p[0].tolist() == list(range(n * n))
    rows = [tuple(r) for r in p.tolist()]
    for s in range(8):
        for t in range(8):
            assert tuple(p[t][p[s]].tolist()) in rows  # sigma_t after sigma_s is one of the eight
    # the definition, spelt out on one square off every axis of symmetry: (r, c) = (0, 1)
    want = [(0, 1), (1, 0), (n - 1, 1), (n - 2, 0), (0, n - 2), (1, n - 1), (n - 1, n - 2), (n - 2, n - 1)]
    assert [divmod(int(p[s][1]), n) for s in range(8)] == want


@pytest.mark.parametrize("n", SIZES)
def test_masks_against_the_reference(hostlib, n):  # noqa: F811
    gen = np.random.default_rng(n)
    W = rr.nwords(n)
    arr = gen.integers(0, 2 ** 64, size=(16, 3, W), dtype=np.uint64)  # bits off the board too: they are dropped
    sym = (np.arange(16) % 8 + 8 * (np.arange(16) % 3)).astype(np.uint8)
    got = host_masks(hostlib, n, sym, arr)
    np.testing.assert_array_equal(got, rr.symmetry_masks(n, sym, arr))
    board = (1 << (n * n)) - 1
    for i in range(16):
        for p in range(3):
            assert bin(rr.to_int(got[i, p])).count("1") == bin(rr.to_int(arr[i, p]) & board).count("1")


@pytest.mark.parametrize("n", SIZES)
def test_legal_moves_commute_with_the_symmetries(hostlib, n):  # noqa: F811
    """Random positions (every square empty, the mover's or the opponent's): the oracle's legal moves of the
    transformed position are the transformed legal moves."""
    gen = np.random.default_rng(100 + n)
    W, nn, E = rr.nwords(n), n * n, 12
    cell = gen.integers(0, 3, size=(E, nn))
    mover = np.zeros((E, W), dtype=np.uint64)
    opp = np.zeros((E, W), dtype=np.uint64)
    for e in range(E):
        mover[e] = rr.to_words(sum(1 << a for a in range(nn) if cell[e, a] == 1), W)
        opp[e] = rr.to_words(sum(1 << a for a in range(nn) if cell[e, a] == 2), W)
    legal = oracle.legal(n, mover, opp)
    assert legal.any()
    planes = np.stack([mover, opp, legal], axis=1)
    for s in range(8):
        sym = np.full(E, s, dtype=np.uint8)
        for t in (host_masks(hostlib, n, sym, planes), rr.symmetry_masks(n, sym, planes)):
            np.testing.assert_array_equal(oracle.legal(n, np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1])),
                                          t[:, 2], err_msg="n %d symmetry %d" % (n, s))
