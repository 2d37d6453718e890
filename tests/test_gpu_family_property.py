"""The search families on ARBITRARY positions, at all 13 board sizes: oth_playouts
(ROOT and MOVES), oth_mcts, oth_puct_begin / _advance / _result, the batch calls,
oth_puct_pick / oth_step / oth_puct_reroot, and oth_solve / oth_search, against
their plain-Python references on the same state.  Every comparison is exact
equality.

The positions are those of tests/test_gpu_property.py's generator (random
disjoint disc masks, either side to move, no board flagged terminated), which
random play from the start never gives the families' own tests: live boards whose
mover has no move while the opponent has one, live boards where nobody can move,
lopsided boards that pass again and again.  On top, every third board's stored
mask is narrowed to a subset of its legal squares and one board's is emptied.

Coverage comes from the fixed table of tests/family_cases.py -- every size x four
density bands; tests/test_family_census.py asserts on the references alone, without
a GPU, what the table holds.  A small hypothesis layer (derandomized, no example
database) draws further sizes, seeds and densities through the same checks."""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import family_cases as fc
import playout_ref as pr
import test_gpu_mcts as tgm
import test_gpu_puct as tgp
import test_gpu_puct_batch as tgpb
import test_gpu_puct_play as tgpp
import test_gpu_search as tgsh
import test_gpu_solve as tgso
from test_gpu_puct import load, make_env, torch_cuda  # noqa: F401  (the fixture)
from test_search_host import host_search, searchlib  # noqa: F401  (the fixture)
from test_solve_host import host_solve, hostlib  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

E = fc.ARB_E
SIZES = fc.ALL_SIZES
assert SIZES == [4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
SETTINGS = dict(max_examples=12, deadline=None, derandomize=True, database=None,
                suppress_health_check=[HealthCheck.too_slow, HealthCheck.function_scoped_fixture])
table = pytest.mark.parametrize("row", fc.TABLE, ids=fc.row_id)
solved = pytest.mark.parametrize("row", [r for k, r in enumerate(fc.TABLE) if k % len(fc.BANDS) in fc.SOLVED_BANDS],
                                 ids=fc.row_id)
position = dict(n=st.sampled_from(SIZES), seed=st.integers(0, 2 ** 31 - 1), db=st.floats(0.0, 0.7), dw=st.floats(0.0, 0.7))


# ------------------------------------------------------------ the checks: one table row or one drawn example
def check_playouts(torch, row):
    n, k = row[0], fc.ARB_KEY
    s = fc.row_state(row)
    env = make_env(E, n, env_id_base=k["id_base"])
    load(torch, env, s)
    for per_move, R in fc.ARB_PLAYOUTS:
        want_wdl, want_score = fc.arb_playouts(row, per_move, R)
        out = env.playouts(R, per_move=per_move, seed=k["seed"], id_key=k["id_key"], counter=k["counter"], score=True,
                           best=per_move)
        what = "MOVES" if per_move else "ROOT"
        np.testing.assert_array_equal(out[0].cpu().numpy(), want_wdl, err_msg=what + " wdl")
        np.testing.assert_array_equal(out[1].cpu().numpy(), want_score, err_msg=what + " score")
        if per_move:
            np.testing.assert_array_equal(out[2].cpu().numpy(), pr.best_moves(s, want_wdl), err_msg="best")
    env.close()


def check_mcts(torch, row):
    n = row[0]
    I, R, C, T = fc.ARB_MCTS
    res = fc.arb_mcts(row)
    env = tgm.make_env(E, n)
    load(torch, env, fc.row_state(row))
    got = env.mcts(I, playouts=R, c=C / 256.0, max_tree_nodes=T, **tgm.KEY, **tgm.ALL)
    for name, g, w in zip(tgm.NAMES, got, res.outputs()):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=name)
    env.close()


def check_puct(torch, row):
    """begin, the advances and result, the leaves compared after every call."""
    n = row[0]
    sims, C, T = fc.ARB_PUCT
    run = fc.arb_puct(row)
    env = make_env(E, n)
    load(torch, env, fc.row_state(row))
    trace, outs = tgp.hash_search(torch, env, n, sims, C, T, layout=None)
    tgp.same_trace(trace, run.leaves)
    tgp.same_outputs(outs, run.outputs)
    env.close()


def check_batch(torch, row):
    """The batch calls until no slot holds a leaf, the E K rows compared after every launch."""
    n = row[0]
    sims, C, T, K = fc.ARB_BATCH
    run = fc.arb_batch(row)
    env = make_env(E, n)
    load(torch, env, fc.row_state(row))
    trace, outs = tgpb.hash_search(torch, env, n, sims, C, T, K)
    tgpb.same_trace(trace, run.leaves)
    tgpb.same_outputs(outs, run.outputs)
    env.close()


def check_game(torch, row):
    """Three moves of begin / advances / pick / oth_step / re-root, everything compared after every call."""
    n = row[0]
    S, M, C, T = fc.ARB_GAME
    game = fc.arb_game(row)
    env = make_env(E, n, seed=3)
    load(torch, env, fc.row_state(row))
    tgpp.play(torch, env, game, (n, E, S, M, C, T))
    env.close()


def check_solve(torch, lib, row):
    n = row[0]
    s, res, me = fc.row_state(row), fc.arb_solve(row), fc.solve_max_e(row[0])
    env = tgso.make_env(E, n)
    tgso.load(torch, env, s)
    tgso.assert_equals_reference(tgso.dev_solve(env, max_empties=me), res, host_solve(lib, s, max_empties=me))
    env.close()


def check_search(torch, lib, row):
    n = row[0]
    s, (res, ws) = fc.row_state(row), fc.arb_search(row)
    env = tgsh.make_env(E, n)
    tgsh.load(torch, env, s)
    tgsh.assert_equals_reference(tgsh.dev_search(env, fc.ARB_SEARCH_DEPTH, ws), res,
                                 host_search(lib, s, fc.ARB_SEARCH_DEPTH, *ws))
    env.close()


# ------------------------------------------------------------ the table
@table
def test_playouts_on_the_table(torch_cuda, row):
    check_playouts(torch_cuda, row)


@table
def test_mcts_on_the_table(torch_cuda, row):
    check_mcts(torch_cuda, row)


@table
def test_puct_on_the_table(torch_cuda, row):
    check_puct(torch_cuda, row)


@table
def test_puct_batch_on_the_table(torch_cuda, row):
    check_batch(torch_cuda, row)


@table
def test_pick_step_reroot_on_the_table(torch_cuda, row):
    check_game(torch_cuda, row)


@solved
def test_solve_on_the_table(torch_cuda, hostlib, row):  # noqa: F811
    check_solve(torch_cuda, hostlib, row)


@solved
def test_search_on_the_table(torch_cuda, searchlib, row):  # noqa: F811
    check_search(torch_cuda, searchlib, row)


# ------------------------------------------------------------ drawn examples: variety on top of the table
@settings(**SETTINGS)
@given(**position)
def test_playouts_on_arbitrary_positions(torch_cuda, n, seed, db, dw):
    check_playouts(torch_cuda, (n, seed, db, dw))


@settings(**SETTINGS)
@given(**position)
def test_mcts_on_arbitrary_positions(torch_cuda, n, seed, db, dw):
    check_mcts(torch_cuda, (n, seed, db, dw))


@settings(**SETTINGS)
@given(**position)
def test_puct_on_arbitrary_positions(torch_cuda, n, seed, db, dw):
    check_puct(torch_cuda, (n, seed, db, dw))
    check_batch(torch_cuda, (n, seed, db, dw))


@settings(**SETTINGS)
@given(**position)
def test_pick_step_reroot_on_arbitrary_positions(torch_cuda, n, seed, db, dw):
    check_game(torch_cuda, (n, seed, db, dw))


@settings(**SETTINGS)
@given(n=st.sampled_from(SIZES), seed=st.integers(0, 2 ** 31 - 1), empty=st.floats(0.0, 0.12), share=st.floats(0.05, 0.95))
def test_solve_and_search_on_arbitrary_positions(torch_cuda, hostlib, searchlib, n, seed, empty, share):  # noqa: F811
    """Nearly full boards of any balance: `empty` of the squares empty, `share` of the discs black."""
    row = (n, seed, (1.0 - empty) * share, (1.0 - empty) * (1.0 - share))
    check_solve(torch_cuda, hostlib, row)
    check_search(torch_cuda, searchlib, row)
