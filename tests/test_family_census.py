"""The arbitrary-position table of tests/family_cases.py, by the references alone:
per board size, over the four density bands together, the positions and the
references' own runs hold what tests/test_gpu_family_property.py is there to put
in front of the device -- stuck movers, boards where nobody can move, game ends
and passes inside the trees, kept and fresh re-roots.  Runs without a GPU."""
import numpy as np
import pytest

import family_cases as fc
import mcts_ref as mr
import puct_ref as pf
from test_search_host import assert_equals_reference as search_equals_reference
from test_search_host import host_search, searchlib  # noqa: F401  (the fixture)
from test_solve_host import assert_equals_reference as solve_equals_reference
from test_solve_host import host_solve, hostlib  # noqa: F401  (the fixture)


def rows_of(n):
    rows = [r for r in fc.TABLE if r[0] == n]
    assert len(rows) == len(fc.BANDS)
    return rows


def test_the_table_covers_every_size_and_band():
    assert sorted({r[0] for r in fc.TABLE}) == list(range(4, 17)) and len(fc.TABLE) == 13 * 4
    assert fc.ARB_E % 8 != 0 and 24 <= fc.ARB_E <= 40
    for n, seed, db, dw in fc.TABLE:
        assert 0 <= db and 0 <= dw and db + dw <= 1.0
    for n in fc.ALL_SIZES:
        t = sum(fc.densities(n, "near_full"))
        assert 0.9 <= t <= 0.97


def test_the_generator_is_the_property_tests():
    """family_cases.arbitrary with 96 boards is test_gpu_property._positions."""
    import test_gpu_property as tp
    for n, seed, db, dw in ((8, 5, 0.3, 0.4), (13, 77, 0.02, 0.9), (15, 3, 0.5, 0.5)):
        a, b = fc.arbitrary(n, tp.E, seed, db, dw), tp._positions(n, seed, db, dw)
        for x, y in ((a.boards, b.boards), (a.meta, b.meta), (a.legal, b.legal)):
            np.testing.assert_array_equal(x, y)


def test_narrowing_keeps_to_the_legal_mask():
    for row in fc.TABLE[::5]:
        n, seed, db, dw = row
        full, s = fc.arbitrary(n, fc.ARB_E, seed, db, dw), fc.row_state(row)
        np.testing.assert_array_equal(s.boards, full.boards)
        np.testing.assert_array_equal(s.meta, full.meta)
        assert not (s.legal & ~full.legal).any()
        wide = int((fc.sr.legal_rows(full.legal, n * n).sum(1) >= 2).sum())
        emptied = ~s.legal.any(1) & full.legal.any(1)
        assert emptied.sum() == (1 if wide >= 2 else 0)
        assert ((s.legal != full.legal).any(1) & ~emptied).sum() == (wide + 2) // 3  # every third, to a true subset


@pytest.mark.parametrize("n", fc.ALL_SIZES)
def test_host_solve_and_search_on_the_table(hostlib, searchlib, n):  # noqa: F811
    """The near-full and the full band: the host builds of the solver and of the search equal the references there, so
    the device's test may hold `nodes` to them; and the band gives the solver boards to value."""
    exact = 0
    for k in fc.SOLVED_BANDS:
        row = rows_of(n)[k]
        s, me = fc.row_state(row), fc.solve_max_e(n)
        res = fc.arb_solve(row)
        solve_equals_reference(host_solve(hostlib, s, max_empties=me), res)
        exact += int((res.status == fc.sr.EXACT).sum())
        res, ws = fc.arb_search(row)
        search_equals_reference(host_search(searchlib, s, fc.ARB_SEARCH_DEPTH, *ws), res)
    assert exact >= 5, "the near-full band gives the solver fewer than five boards within its empties"


@pytest.mark.parametrize("n", fc.ALL_SIZES)
def test_census(n):
    with_moves = stuck = nobody = 0
    mcts_ends = mcts_passes = puct_ends = puct_passes = kept = fresh = batch_ends = 0
    for row in rows_of(n):
        _, seed, db, dw = row
        s = fc.arbitrary(n, fc.ARB_E, seed, db, dw)
        assert not (s.meta & 2).any()  # live, whoever can move
        mine, theirs = fc.kinds(s)
        np.testing.assert_array_equal(mine, s.legal.any(1))
        with_moves += int(mine.sum())
        stuck += int((~mine & theirs).sum())
        nobody += int((~mine & ~theirs).sum())
        res = fc.arb_mcts(row)
        mcts_ends += int(res.terminated_stops.sum())
        mcts_passes += int(res.pass_children.sum())
        assert set(res.status.tolist()) <= {mr.DONE, mr.NO_MOVE}
        run = fc.arb_puct(row)
        puct_ends += run.counters["terminal_leaves"]
        puct_passes += run.counters["pass_children"]
        batch_ends += int((np.concatenate([lv[0] for lv in fc.arb_batch(row).leaves]) == pf.TERMINAL).sum())
        game = fc.arb_game(row)
        kept += game.counters["kept"]
        fresh += game.counters["fresh"]
    assert with_moves > 0, "no board with moves"
    assert stuck > 0, "no live board whose mover is stuck while the opponent has a move"
    assert nobody > 0, "no live board where neither side has a move"
    assert mcts_ends > 0 and mcts_passes > 0, "mcts: no terminated stop or no pass child"
    assert puct_ends > 0 and puct_passes > 0, "puct: no terminal leaf or no pass child"
    assert batch_ends > 0, "batch: no terminal leaf"
    assert kept > 0 and fresh > 0, "re-root: no kept or no fresh board"
