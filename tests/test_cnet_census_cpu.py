"""What the case table of tests/cnet_cases.py is there for, held of the reference's own
numbers: saturation cannot hide a wrong sum (at every layer of every case at least a
quarter of the activations lie strictly between 0 and 127; in at least half the rows
with two or more legal squares the priors are not one-hot), the hand-made rows are
what they say, and the reference's float64 matrix product is its int64 sum."""
import numpy as np
import pytest

import cnet_cases as cc
import cnet_ref as cr
import net_ref as nr


@pytest.mark.parametrize("i", range(len(cc.TABLE)), ids=cc.IDS)
def test_activations_and_priors_are_spread(i):
    c = cc.case(i)
    assert len(c.census) == 2 + 2 * c.B  # the stem, every conv, the head's features
    assert min(c.census) >= 0.25, c.census
    lg = nr.bits(c.legal, c.nn)
    many = lg.sum(axis=1) >= 2
    if many.any():
        one_hot = (c.priors[many] > 0).sum(axis=1) == 1
        assert (~one_hot).sum() * 2 >= many.sum(), (int(one_hot.sum()), int(many.sum()))
    assert (c.priors[lg == 0] == 0).all()
    rows = lg.sum(axis=1) > 0
    assert (abs(c.priors[rows].sum(axis=1) - 65535) <= c.nn).all()  # each prior is rounded once
    assert (c.priors[~rows] == 0).all()
    assert all(0 <= s <= 24 for s in [c.shift_stem, c.shift_head, c.policy_shift, c.value_shift] + c.shifts)


@pytest.mark.parametrize("n", (4, 5, 16))
def test_the_layout_case(n):
    """One feature a row: every row's logits are its own, so each (plane, square) reaches the head by its own taps;
    the activations are spread at every layer, so a wrong sum shows."""
    c = cc.layout_case(n)
    print(c.census)
    assert c.R == 3 * c.nn + 1 and len({c.logits[f].tobytes() for f in range(c.R)}) == c.R
    assert min(c.census) >= 0.25, c.census
    assert len(set(c.values.tolist())) > c.nn // 2


def test_the_table():
    assert cc.TABLE == [(4, 1, 1, 64), (5, 17, 1, 64), (6, 15, 2, 128), (8, 67, 3, 64), (8, 33, 8, 128),
                        (10, 19, 2, 64), (13, 5, 1, 128), (16, 18, 2, 128), (16, 3, 1, 64)]
    assert {nr.nwords(c[0]) for c in cc.TABLE} == {1, 2, 3, 4}
    values = np.concatenate([cc.case(i).values for i in (3, 4)])
    assert len(set(values.tolist())) > 20 and (abs(values) < 32768).any()


def test_hand_made_rows():
    for n in (4, 5, 8, 16):
        nn = n * n
        boards, meta, legal = cc.hand_rows(n)
        x = nr.features(n, boards, meta, legal).reshape(4, 3, n, n)
        edge = np.ones((n, n), bool)
        edge[1:-1, 1:-1] = False
        assert (x[0, 0][edge] == 1).all() and x[0, 0].sum() == edge.sum()  # the mover (white) on every edge and corner
        assert (x[2, 1][edge] == 1).all() and x[2, 2].sum() == nn - x[2, 0].sum() - x[2, 1].sum()
        assert (x[1, 0] + x[1, 1] == 1).all() and x[1, 2].sum() == 0  # a full board, no legal square
        assert x[3, 2].sum() == 0 and x[3, 0][0, 0] == 1 and x[3, 1][n - 1, n - 1] == 1
        assert [int(m) & 1 for m in meta] == [1, 0, 0, 1]
    c = cc.case(3)
    lg = nr.bits(c.legal, c.nn)
    assert (lg.sum(axis=1) == 0).any() and {int(m) & 1 for m in c.meta[:c.R - 4]} == {0, 1}  # games: both movers


def test_float64_products_are_the_int64_sums():
    c = cc.case(1)
    exact = cr.ConvNet(c.n, *cc.net_args(c), exact=True)
    np.testing.assert_array_equal(exact.logits(c.boards, c.meta, c.legal), c.logits)
    # the largest sums the format allows: every weight -128 or 127 on activations of 127
    gen = np.random.default_rng(1)
    w = np.where(gen.random((128, 128, 3, 3)) < 0.5, -128, 127).astype(np.int64)
    x = np.full((2, 128, 4, 4), 127, np.int64)
    b = np.full(128, cr.BIAS_MAX, np.int64)
    np.testing.assert_array_equal(cr.conv(w, b, x), cr.conv(w, b, x, exact=True))
    low = cr.conv(np.full_like(w, -128), -b, x)  # the bound of the header: 9 * 128 * 127 * 128 beside a bias of 2^30
    assert low.min() == -cr.BIAS_MAX - 9 * 128 * 127 * 128 and 9 * 128 * 127 * 128 < 2 ** 25
