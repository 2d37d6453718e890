"""oth_mcts / VecOthelloEnv.mcts / MCTSPolicy on the device against the plain
Python integers of tests/mcts_ref.py (the header's algorithm on oracle.step and
oracle.rollout).  Every comparison with the reference is exact equality."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

import mcts_ref as mr
from oracle import oracle

pytestmark = pytest.mark.gpu

NAMES = ("visits", "wins2", "best", "tree_nodes", "status")
KEY = dict(seed=mr.SEED, id_key=mr.ID_KEY, counter=mr.COUNTER)
ALL = dict(wins2=True, best=True, tree_nodes=True, status=True)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def make_env(E, n, seed=0, id_base=mr.ID_BASE, **kw):
    from gymothelloenv_amd import VecOthelloEnv
    return VecOthelloEnv(E, board_size=n, seed=seed, env_id_base=id_base, device="cuda:0", **kw)


def load(torch, env, s):
    env.set_state(torch.from_numpy(s.boards.view(np.int64)).cuda(), torch.from_numpy(s.meta.view(np.int16)).cuda(),
                  torch.from_numpy(s.legal.view(np.int64)).cuda())


def state_np(env):
    b, m, lg = env.get_state()
    return (b.cpu().numpy().view(np.uint64), m.cpu().numpy().view(np.uint16), lg.cpu().numpy().view(np.uint64))


def subset(s, rows):
    t = oracle.State(s.n, len(rows))
    t.boards[:], t.meta[:], t.legal[:] = s.boards[rows], s.meta[rows], s.legal[rows]
    return t


def raw_mcts(torch, env, I, R, C, T, sentinel):
    """oth_mcts through the C ABI into outputs pre-filled with a sentinel."""
    from gymothelloenv_amd import _lib as L
    E, nn = env.num_envs, env.board_size ** 2
    need = ctypes.c_uint64(0)
    L.check(env._lib.oth_mcts_workspace_bytes(env.board_size, E, T, ctypes.byref(need)))
    ws = torch.full((need.value,), 0xA5, dtype=torch.uint8, device="cuda:0")  # no initialising needed: garbage
    outs = [torch.full((E, nn), sentinel, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    outs += [torch.full((E,), sentinel, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    outs.append(torch.full((E,), sentinel & 0xff, dtype=torch.uint8, device="cuda:0"))
    p = L.OthMctsParams(I, R, C, T, mr.SEED, mr.ID_KEY, mr.COUNTER)
    ptrs = [ctypes.c_void_p(t.data_ptr()) for t in outs]
    L.check(env._lib.oth_mcts(env._h, ctypes.byref(p), ctypes.c_void_p(ws.data_ptr()), ws.numel(), *ptrs,
                              env._stream()), "oth_mcts")
    return [t.cpu().numpy() for t in outs]


@pytest.mark.parametrize("c", mr.CASES, ids=lambda c: "n%d-E%d-I%d-R%d-C%d-T%d" % c)
def test_exact_against_the_reference(torch_cuda, c):
    torch = torch_cuda
    n, E, I, R, C, T = c
    s, res = mr.case(c)
    mr.check_case(c, res)
    env = make_env(E, n, seed=3)
    load(torch, env, s)
    before = state_np(env)
    ply, cnt, cnt_vs, calls = env.ply_counter, env.counts().clone(), env.counts_vs().clone(), env.playout_counter
    got = env.mcts(I, playouts=R, c=C / 256.0, max_tree_nodes=T, **KEY, **ALL)
    assert got[0].shape == (E, n * n) and got[0].dtype == torch.int32 and got[4].dtype == torch.uint8
    for name, g, w in zip(NAMES, got, res.outputs()):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=name)
    # sentinel-filled outputs are fully overwritten, from a workspace of garbage
    for name, g, w in zip(NAMES, raw_mcts(torch, env, I, R, C, T, 0x7a7a7a7a), res.outputs()):
        np.testing.assert_array_equal(g, w, err_msg="sentinel " + name)
    only = env.mcts(I, playouts=R, c=C / 256.0, max_tree_nodes=T, **KEY)  # the optional outputs NULL
    assert torch.equal(only, got[0])
    # nothing of the handle is written
    for x, y in zip(before, state_np(env)):
        np.testing.assert_array_equal(x, y)
    assert env.ply_counter == ply and env.playout_counter == calls
    assert torch.equal(env.counts(), cnt) and torch.equal(env.counts_vs(), cnt_vs)
    env.close()


def test_determinism_and_independence(torch_cuda):
    torch = torch_cuda
    c = mr.CASES[1]
    n, E, I, R, C, T = c
    assert (n, E) == (6, 12)
    s, res = mr.case(c)
    kw = dict(playouts=R, c=C / 256.0, max_tree_nodes=T, **KEY, **ALL)
    env = make_env(E, n)
    load(torch, env, s)
    a, b = env.mcts(I, **kw), env.mcts(I, **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    env.close()
    # boards 4..8 alone, with their global ids
    part = make_env(5, n, id_base=mr.ID_BASE + 4)
    load(torch, part, subset(s, list(range(4, 9))))
    for name, g, w in zip(NAMES, part.mcts(I, **kw), res.outputs()):
        np.testing.assert_array_equal(g.cpu().numpy(), w[4:9], err_msg=name)
    part.close()
    # any order of the boards, each keeping its global id: one handle a board
    for e in np.random.RandomState(5).permutation(E):
        one = make_env(1, n, id_base=mr.ID_BASE + int(e))
        load(torch, one, subset(s, [int(e)]))
        for name, g, w in zip(NAMES, one.mcts(I, **kw), res.outputs()):
            np.testing.assert_array_equal(g.cpu().numpy(), w[e:e + 1], err_msg="%s of board %d" % (name, e))
        one.close()


def test_counters_and_seeds(torch_cuda):
    torch = torch_cuda
    env = make_env(9, 8, seed=21)
    env.reset()
    env.step_policy("random", 10, record=False)
    kw = dict(playouts=8, wins2=True)
    a = env.mcts(32, seed=1, id_key=2, counter=3, **kw)[1]
    assert torch.equal(a, env.mcts(32, seed=1, id_key=2, counter=3, **kw)[1])
    assert not torch.equal(a, env.mcts(32, seed=1, id_key=2, counter=4, **kw)[1])
    assert not torch.equal(a, env.mcts(32, seed=2, id_key=2, counter=3, **kw)[1])
    assert not torch.equal(a, env.mcts(32, seed=1, id_key=3, counter=3, **kw)[1])
    assert env.playout_counter == 0  # explicit counters leave it alone
    d0 = env.mcts(32, **kw)[1]
    assert env.playout_counter == 1
    from gymothelloenv_amd.vec_env import PLAYOUT_SEED_XOR
    assert torch.equal(d0, env.mcts(32, seed=21 ^ PLAYOUT_SEED_XOR, counter=0, **kw)[1])
    best = env.mcts(32, seed=1, id_key=2, counter=3, best=True)[1]
    assert torch.equal(env.mcts_actions(32, seed=1, id_key=2, counter=3), best)
    assert torch.equal(env.mcts_actions(32, seed=1, id_key=2, counter=3, best=False, status=True), best)
    env.close()


def test_argument_errors_on_a_live_handle(torch_cuda):
    from gymothelloenv_amd import OthelloLibError
    env = make_env(4, 8)
    env.reset()
    for kw, word in ((dict(iterations=0), "iterations"), (dict(iterations=65536), "iterations"),
                     (dict(iterations=8, playouts=65), "playouts"), (dict(iterations=8, c=256.5), "c_explore"),
                     (dict(iterations=8, max_tree_nodes=63), "max_tree_nodes"),
                     (dict(iterations=8, counter=2 ** 56), "counter")):
        with pytest.raises(OthelloLibError, match=word):
            env.mcts(**kw)
    env.close()


def test_graph_capture_repeats_the_same_search(torch_cuda):
    """The call only enqueues, so a HIP graph captures it once its workspace is warm."""
    torch = torch_cuda
    env = make_env(9, 8)
    env.reset()
    env.step_policy("random", 12, record=False)
    kw = dict(playouts=8, seed=1, counter=2, **ALL)
    want = env.mcts(48, **kw)  # (warms the workspace)
    ply = env.ply_counter
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # records only
        got = env.mcts(48, **kw)
    for _ in range(2):
        for t in got:
            t.fill_(119)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y)
    assert env.ply_counter == ply
    env.close()


def test_mcts_policy_replays_its_game(torch_cuda):
    import gymothelloenv_amd as g
    games = []
    for _ in range(2):
        opp = g.RandomPolicy(seed=1)
        env = g.OthelloEnv(white_policy=opp, black_policy=opp, protagonist=g.WHITE_DISK, board_size=6)
        pol = g.MCTSPolicy(iterations=32, playouts=4, seed=99)
        moves = []
        with contextlib.redirect_stdout(io.StringIO()):
            obs = env.reset()
            pol.reset(env)
            done = False
            while not done:
                assert pol.counter == len(moves)
                legal = list(env.possible_moves)
                a = pol.get_action(obs)
                want = int(env.env._vec.mcts_actions(32, playouts=4, seed=99, counter=len(moves)).cpu()[0])
                assert a == want and a in legal
                obs, r, done, _ = env.step(a)
                moves.append(a)
        assert done and len(moves) >= 4
        games.append(moves)
    assert games[0] == games[1]
    base = g.OthelloBaseEnv(board_size=6, mute=True)  # not reset: no possible moves
    pol.reset(base)
    with pytest.raises(ValueError, match="no possible moves"):
        pol.get_action(None)
    pol.seed(5)
    assert pol.counter == 0


def test_mcts_beats_random_play(torch_cuda):
    """64 6x6 games as black against the device's random policy, one mcts call per
    move (I = 64, R = 8): more wins than losses.  A sanity condition with a wide
    margin, not a strength measurement (DESIGN.md section 5 has the measured rate)."""
    torch = torch_cuda
    E, n = 64, 6
    env = make_env(E, n, seed=11, id_base=0)
    env.reset_vs("random", protagonist=-1)
    done = torch.zeros(E, dtype=torch.bool, device="cuda:0")
    for move in range(n * n):
        if bool(done.all()):
            break
        a = env.mcts_actions(64, playouts=8, seed=5, counter=move)
        _, _, d, _ = env.step_vs(a, "random", observe=False)
        done |= d
    assert bool(done.all())
    discs = env.count_disks().cpu().numpy()  # (white, black)
    wins, losses = int((discs[:, 1] > discs[:, 0]).sum()), int((discs[:, 1] < discs[:, 0]).sum())
    print("MCTS (I = 64, R = 8) as black against random on 64 6x6 boards: %d wins, %d losses" % (wins, losses))
    assert wins > losses
    env.close()
