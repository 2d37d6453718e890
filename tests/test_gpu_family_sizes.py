"""Every search family on the device at every board size its own test file leaves
out: oth_playouts, oth_solve, oth_search, oth_play_search / oth_step_vs_search,
oth_mcts and the oth_puct family (begin / advance / result, pick and re-root in
both mappings, the batch calls, the leaves' observation).

NEW_SIZES = 5, 7, 9, 11, 12, 13, 14, 15 (tests/family_cases.py): with the
families' own files every family runs at every N from 4 to 16.  12 and 13 take
three words a board, 14 and 15 four with a partly used last word, 9 and 11 two
with rows that straddle bit 64 otherwise than 10's, 5 and 7 one.  The checks are
the families' own -- exact equality with the plain-Python references, `nodes`
equal to the host builds (held to the references at these sizes by
tests/test_*_host.py) -- at the smallest shapes that still reach each family's
lane and wave mappings; every case first states, on the reference alone, what it
is there to reach."""
import numpy as np
import pytest

import family_cases as fc
import playout_ref as pr
import puct_play_ref as pp
import puct_ref as pf
import search_ref as sh
import test_gpu_mcts as tgm
import test_gpu_play_search as tgps
import test_gpu_playouts as tgpo
import test_gpu_puct as tgp
import test_gpu_puct_batch as tgpb
import test_gpu_puct_play as tgpp
import test_gpu_search as tgsh
import test_gpu_solve as tgso
from test_gpu_puct import LAYOUTS, leaves_np, load, make_env, torch_cuda  # noqa: F401  (the fixture)
from test_gpu_puct_play import lane_lib  # noqa: F401  (the fixture)
from test_search_host import host_search, searchlib  # noqa: F401  (the fixture)
from test_solve_host import hostlib  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

NEW_SIZES = fc.NEW_SIZES
assert NEW_SIZES == [5, 7, 9, 11, 12, 13, 14, 15]


# ------------------------------------------------------------ oth_playouts
def root_playouts(torch, n, E, Rs):
    s = tgpo.positions(n, E)
    pr.check_positions(s)  # a fresh, a terminated, a one-empty and a forced-pass board, games of several lengths
    env = tgpo.make_env(E, n, id_base=tgpo.ID_BASE)
    tgpo.load(torch, env, s)
    key = dict(seed=tgpo.SEED, id_key=tgpo.ID_KEY, counter=tgpo.COUNTER)
    for R in Rs:
        wdl, score = env.playouts(R, score=True, **key)
        want_wdl, want_score = pr.replay(s, False, R, tgpo.SEED, tgpo.ID_KEY, tgpo.ID_BASE, tgpo.COUNTER)
        assert (want_wdl.sum(1) == np.where((s.meta & 2) == 0, R, 0)).all() and len(np.unique(want_score)) > 3
        np.testing.assert_array_equal(wdl.cpu().numpy(), want_wdl, err_msg="R = %d" % R)
        np.testing.assert_array_equal(score.cpu().numpy(), want_score, err_msg="R = %d" % R)
    env.close()


@pytest.mark.parametrize("n", NEW_SIZES)
def test_playouts_root(torch_cuda, n):
    """R = 5: several boards share a wave; R = 130: the wave-uniform row path."""
    root_playouts(torch_cuda, n, 9, (5, 130))


def test_playouts_root_more_boards_than_a_wave_at_a_three_word_stride(torch_cuda):
    root_playouts(torch_cuda, 12, 70, (3,))


@pytest.mark.parametrize("n", NEW_SIZES)
def test_playouts_moves(torch_cuda, n):
    torch = torch_cuda
    E, R, nn = 9, 3, n * n
    s = tgpo.positions(n, E)
    pr.check_positions(s)
    env = tgpo.make_env(E, n, id_base=tgpo.ID_BASE)
    tgpo.load(torch, env, s)
    wdl, score, best = env.playouts(R, per_move=True, seed=tgpo.SEED, id_key=tgpo.ID_KEY, counter=tgpo.COUNTER, score=True,
                                    best=True)
    want_wdl, want_score = pr.replay(s, True, R, tgpo.SEED, tgpo.ID_KEY, tgpo.ID_BASE, tgpo.COUNTER)
    want_best = pr.best_moves(s, want_wdl)
    lb = np.stack([pr.legal_bool(s.legal[e], nn) for e in range(E)]) & ((s.meta & 2) == 0)[:, None]
    assert (want_wdl.sum(2) == np.where(lb, R, 0)).all() and want_best[1] == -1 and (want_best[[0, 2, 3]] >= 0).all()
    assert s.boards[:, s.W - 1].any() and s.boards[:, 2 * s.W - 1].any(), "no discs of both colours in the last word"
    np.testing.assert_array_equal(wdl.cpu().numpy(), want_wdl)
    np.testing.assert_array_equal(score.cpu().numpy(), want_score)
    np.testing.assert_array_equal(best.cpu().numpy(), want_best)
    env.close()


# ------------------------------------------------------------ oth_solve, oth_search
@pytest.mark.parametrize("n", fc.NEW_SIZES_SOLVE)  # (5 x 5 runs in test_gpu_solve.py)
def test_solve(torch_cuda, hostlib, n):  # noqa: F811
    """test_gpu_solve.test_exact: 37 boards with the eight specials (check_batch), value, best, move_values and status
    equal to the minimax, nodes equal to the host build and within the minimax's."""
    tgso.test_exact(torch_cuda, hostlib, n, fc.solve_max_e(n))


@pytest.mark.parametrize("n", fc.NEW_SIZES_SOLVE)  # (5 x 5 runs in test_gpu_search.py)
def test_search(torch_cuda, searchlib, n):  # noqa: F811
    torch = torch_cuda
    E = 74
    sh.reference(n, E, sh.BUILD_DEPTH, "default")  # check_batch: the nine specials are in the batch
    env = tgsh.make_env(E, n)
    for depth in (1, 3):
        s, res, ws = sh.reference(n, E, depth, fc.SEARCH_WSET)
        assert ws[1] != 0 and (res.status == sh.DONE).sum() > 30
        tgsh.load(torch, env, s)
        got = tgsh.dev_search(env, depth, ws)
        tgsh.assert_equals_reference(got, res, host_search(searchlib, s, depth, *ws))
    env.close()


# ------------------------------------------------------------ oth_play_search, oth_step_vs_search
@pytest.mark.parametrize("n", NEW_SIZES)
def test_play_moves_are_the_references(torch_cuda, searchlib, n):  # noqa: F811
    """(play_reference asserts fallbacks, passes, endgame-mode moves and game ends in the run.)"""
    tgps.test_play_moves_are_the_references(torch_cuda, searchlib, n)


@pytest.mark.parametrize("first", ["protagonist", "opponent"])
@pytest.mark.parametrize("n", NEW_SIZES)
def test_vs_moves_are_the_references(torch_cuda, searchlib, n, first):  # noqa: F811
    tgps.test_vs_moves_are_the_references(torch_cuda, searchlib, n, first)


@pytest.mark.parametrize("n", [7, 12, 15])
def test_play_control_flow_is_the_oracles(torch_cuda, n):
    """Auto-reset and six opening plies, through the greedy-equivalent policy."""
    tgps.test_play_control_flow_is_the_oracles(torch_cuda, n, 4, 6)


@pytest.mark.parametrize("n", [7, 12, 15])
def test_vs_control_flow_is_the_oracles(torch_cuda, n):
    tgps.test_vs_control_flow_is_the_oracles(torch_cuda, n, "mixed", 4, 6)


# ------------------------------------------------------------ oth_mcts
@pytest.mark.parametrize("c", [fc.mcts_case(n) for n in NEW_SIZES] + [fc.mcts_case(n, full=True) for n in fc.MCTS_FULL],
                         ids=lambda c: "n%d-E%d-I%d-R%d-C%d-T%d" % c)
def test_mcts(torch_cuda, c):
    """(mcts_ref.check_case: a terminated stop, a pass child, depth >= 3, and the tree fills exactly when T = N*N.)"""
    tgm.test_exact_against_the_reference(torch_cuda, c)


# ------------------------------------------------------------ oth_puct_begin / _advance / _result
@pytest.mark.parametrize("c", [fc.puct_case(n) for n in NEW_SIZES] + [fc.puct_case(n, full=True) for n in fc.PUCT_FULL],
                         ids=lambda c: pf.CASE_ID % c)
def test_puct(torch_cuda, c):
    """The leaves after begin and after every advance, then the result (puct_ref.check_case: a pass child, depth >= 3,
    clamped priors and values, floor and tie selections, VALUE leaves exactly when T = N*N)."""
    tgp.test_exact_against_the_reference(torch_cuda, c)


# ------------------------------------------------------------ oth_puct_pick, oth_puct_reroot
@pytest.mark.parametrize("mapping", ["wave", "lane"])
@pytest.mark.parametrize("c", [fc.play_case(n) for n in NEW_SIZES], ids=lambda c: pp.CASE_ID % c)
def test_puct_pick_and_reroot(torch_cuda, lane_lib, c, mapping):  # noqa: F811
    fc.check_play_case(c, pp.case(c)[1])
    tgpp.test_exact_against_the_reference(torch_cuda, lane_lib, c, mapping)


# ------------------------------------------------------------ the batch calls
@pytest.mark.parametrize("c", [fc.batch_case(n) for n in NEW_SIZES] + [fc.BATCH_WIDE], ids=lambda c: tgpb.pb.CASE_ID % c)
def test_puct_batch(torch_cuda, c):
    s, run, census = fc.batch_run(c)
    fc.check_batch_case(c, run, census)
    tgpb.test_exact_against_the_reference(torch_cuda, c)


# ------------------------------------------------------------ the leaves' observation
def same_observation(torch, other, leaves, layout, dtype, what):
    """obs is oth_observe of a handle set_state'd to the returned boards, meta and legal."""
    other.set_state(leaves.boards, leaves.meta, leaves.legal)
    want = other.observe(layout, dtype)
    assert leaves.obs.dtype == dtype and leaves.obs.shape == want.shape, what
    assert torch.equal(leaves.obs, want), what


@pytest.mark.parametrize("n", fc.OBS_SIZES)
def test_observation_of_the_leaves(torch_cuda, n):
    """N*N % 4 != 0 on one, two and three words: every layout in int8, float32 and bfloat16, at begin, early in the
    search and at its last leaves."""
    torch = torch_cuda
    _, E, _, C, T = c = fc.puct_case(n)
    assert (n * n) % 4 != 0
    s, run = pf.case(c)
    env, other = make_env(E, n), make_env(E, n)
    load(torch, env, s)
    sims = 12
    for layout in LAYOUTS:
        for dtype in (torch.int8, torch.float32, torch.bfloat16):
            leaves = env.puct_begin(c=C / 256.0, max_tree_nodes=T, layout=layout, dtype=dtype)
            for i in range(sims + 1):
                got = leaves_np(leaves)
                if i < sims:  # the leaves are the reference's: expanded nodes, terminal ones, no leaf on board 1
                    for name, g, w in zip(pf.LEAF_NAMES, got, run.leaves[i]):
                        np.testing.assert_array_equal(g, w, err_msg="%s %d" % (name, i))
                if i in (0, 1, 5, sims):
                    same_observation(torch, other, leaves, layout, dtype, (layout, dtype, i))
                if i < sims:
                    priors, values = pf.hash_eval(got[1], got[2], n * n)
                    leaves = env.puct_advance(torch.from_numpy(priors).cuda(), torch.from_numpy(values).cuda(),
                                              more=i < sims - 1)
            assert int(leaves.kind.max()) == pf.NONE
    assert len({lv[1].tobytes() for lv in run.leaves[:sims]}) == sims  # the leaves move on
    env.close()
    other.close()


@pytest.mark.parametrize("n", fc.OBS_SIZES)
def test_observation_of_the_batch_leaves(torch_cuda, n):
    """The same for the E K rows of the batch calls."""
    torch = torch_cuda
    _, E, sims, C, T, K = c = fc.batch_case(n)
    s, run, _ = fc.batch_run(c)
    env, other = make_env(E, n), make_env(E * K, n)
    load(torch, env, s)
    for layout in LAYOUTS:
        for dtype in (torch.int8, torch.float32, torch.bfloat16):
            leaves = env.puct_begin_batch(K, c=C / 256.0, max_tree_nodes=T, layout=layout, dtype=dtype)
            for i in range(7):
                same_observation(torch, other, leaves, layout, dtype, (layout, dtype, i))
                got = leaves_np(leaves)
                for name, g, w in zip(pf.LEAF_NAMES, got, run.leaves[i] if i <= 5 else ()):
                    np.testing.assert_array_equal(g, w, err_msg="%s %d" % (name, i))
                priors, values = pf.hash_eval(got[1], got[2], n * n)
                leaves = env.puct_advance_batch(torch.from_numpy(priors).cuda(), torch.from_numpy(values).cuda(),
                                                sim_limit=sims if i < 5 else 0)
            assert not bool(leaves.kind.any())  # sim_limit = 0: nothing is selected
            same_observation(torch, other, leaves, layout, dtype, (layout, dtype, "end"))
    # more slots than one hold leaves
    assert len(run.leaves) > 6 and all(lv[0].reshape(E, K)[:, 1:].any() for lv in run.leaves[1:6])
    env.close()
    other.close()
