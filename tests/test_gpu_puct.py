"""oth_puct_begin / _advance / _result, VecOthelloEnv.puct_* and PUCTPolicy on the
device against the plain Python integers of tests/puct_ref.py (the header's
algorithm on oracle.step), the leaves compared after every launch.  Every
comparison with the reference is exact equality."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

import puct_ref as pf
from oracle import oracle

pytestmark = pytest.mark.gpu

ALL = dict(value_sums=True, best=True, tree_nodes=True, status=True)
VIEWS = (np.uint8, np.uint64, np.uint16, np.uint64)
LAYOUTS = ("board", "board_legal", "make_state", "absolute", "legal")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def make_env(E, n, seed=0, **kw):
    from gymothelloenv_amd import VecOthelloEnv
    return VecOthelloEnv(E, board_size=n, seed=seed, device="cuda:0", **kw)


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


def leaves_np(leaves):
    return [t.cpu().numpy().view(v) for t, v in zip(leaves[:4], VIEWS)]


def hash_search(torch, env, n, sims, C, T, between=None, **begin):
    """The whole search with the reference's hash evaluator computed from the device's own
    leaves: the leaves after begin and after every advance (numpy), then the outputs."""
    leaves = env.puct_begin(c=C / 256.0, max_tree_nodes=T, **begin)
    trace = [leaves_np(leaves)]
    for i in range(sims):
        if between is not None:
            between(i)
        priors, values = pf.hash_eval(trace[-1][1], trace[-1][2], n * n)
        leaves = env.puct_advance(torch.from_numpy(priors).cuda(), torch.from_numpy(values).cuda(), more=i < sims - 1)
        trace.append(leaves_np(leaves))
    return trace, [t.cpu().numpy() for t in env.puct_result(**ALL)]


def same_trace(got, want, rows=slice(None), what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for name, x, y in zip(pf.LEAF_NAMES, g, w):
            np.testing.assert_array_equal(x, y[rows], err_msg="%s leaf %s after launch %d" % (what, name, i))


def same_outputs(got, want, rows=slice(None), what=""):
    for name, g, w in zip(pf.NAMES, got, want):
        np.testing.assert_array_equal(g, w[rows], err_msg="%s %s" % (what, name))


def raw_search(torch, env, n, sims, C, T, sentinel):
    """The three calls through the C ABI: a workspace of garbage, every output and leaf array
    pre-filled with a sentinel before each call."""
    from gymothelloenv_amd import _lib as L
    E, nn, W = env.num_envs, n * n, env.words
    need = ctypes.c_uint64(0)
    L.check(env._lib.oth_puct_workspace_bytes(n, E, T, ctypes.byref(need)))
    ws = torch.full((need.value,), 0xA5, dtype=torch.uint8, device="cuda:0")
    wsp = ctypes.c_void_p(ws.data_ptr())
    lt = [torch.empty(E, dtype=torch.uint8, device="cuda:0"), torch.empty(E, 2 * W, dtype=torch.int64, device="cuda:0"),
          torch.empty(E, dtype=torch.int16, device="cuda:0"), torch.empty(E, W, dtype=torch.int64, device="cuda:0")]
    lv = L.OthPuctLeaves(lt[0].data_ptr(), lt[1].data_ptr(), lt[2].data_ptr(), lt[3].data_ptr(), None, 0, 0)
    p = L.OthPuctParams(C, T)

    def fill():
        for t in lt:
            t.fill_(sentinel & 0x7f)

    def get():
        return [t.cpu().numpy().view(v) for t, v in zip(lt, VIEWS)]

    fill()
    L.check(env._lib.oth_puct_begin(env._h, ctypes.byref(p), wsp, ws.numel(), ctypes.byref(lv), env._stream()),
            "oth_puct_begin")
    trace = [get()]
    for i in range(sims):
        priors, values = pf.hash_eval(trace[-1][1], trace[-1][2], nn)
        pr, vl = torch.from_numpy(priors).cuda(), torch.from_numpy(values).cuda()
        fill()
        L.check(env._lib.oth_puct_advance(env._h, ctypes.byref(p), wsp, ws.numel(), ctypes.c_void_p(pr.data_ptr()),
                                          ctypes.c_void_p(vl.data_ptr()), int(i < sims - 1), ctypes.byref(lv),
                                          env._stream()), "oth_puct_advance")
        trace.append(get())
    outs = [torch.full((E, nn), sentinel, dtype=torch.int32, device="cuda:0"),
            torch.full((E, nn), sentinel, dtype=torch.int64, device="cuda:0"),
            torch.full((E,), sentinel, dtype=torch.int32, device="cuda:0"),
            torch.full((E,), sentinel, dtype=torch.int32, device="cuda:0"),
            torch.full((E,), sentinel & 0xff, dtype=torch.uint8, device="cuda:0")]
    L.check(env._lib.oth_puct_result(env._h, ctypes.byref(p), wsp, ws.numel(),
                                     *([ctypes.c_void_p(t.data_ptr()) for t in outs] + [env._stream()])),
            "oth_puct_result")
    return trace, [t.cpu().numpy() for t in outs]


@pytest.mark.parametrize("c", pf.CASES, ids=lambda c: pf.CASE_ID % c)
def test_exact_against_the_reference(torch_cuda, c):
    torch = torch_cuda
    n, E, sims, C, T = c
    s, run = pf.case(c)
    pf.check_case(c, run)
    env = make_env(E, n, seed=3)
    load(torch, env, s)
    before = state_np(env)
    ply, cnt, cnt_vs, calls = env.ply_counter, env.counts().clone(), env.counts_vs().clone(), env.playout_counter
    # sentinel-filled outputs and leaves are fully overwritten, from a workspace of garbage
    trace, outs = raw_search(torch, env, n, sims, C, T, 0x7a7a7a7a)
    same_trace(trace, run.leaves, what="raw")
    same_outputs(outs, run.outputs, what="raw")
    # the Python surface
    trace, outs = hash_search(torch, env, n, sims, C, T, layout=None)
    same_trace(trace, run.leaves)
    same_outputs(outs, run.outputs)
    only = env.puct_result()  # the optional outputs NULL
    assert only.dtype == torch.int32 and only.shape == (E, n * n)
    np.testing.assert_array_equal(only.cpu().numpy(), run.outputs[0])
    # nothing of the handle is written
    for x, y in zip(before, state_np(env)):
        np.testing.assert_array_equal(x, y)
    assert env.ply_counter == ply and env.playout_counter == calls
    assert torch.equal(env.counts(), cnt) and torch.equal(env.counts_vs(), cnt_vs)
    env.close()


@pytest.mark.parametrize("c", [pf.CASES[2], pf.CASES[3]], ids=lambda c: pf.CASE_ID % c)
def test_observation_of_the_leaves(torch_cuda, c):
    """obs is oth_observe of a second env set_state'd to the leaf arrays, for every layout and
    three dtypes, at several points of the search (begin, early, the last leaves, all NONE)."""
    torch = torch_cuda
    n, E, sims, C, T = c
    assert n in (8, 10)
    s, run = pf.case(c)
    env, other = make_env(E, n), make_env(E, n)
    load(torch, env, s)
    sims = 12
    for layout in LAYOUTS:
        for dtype in (torch.int8, torch.float32, torch.bfloat16):
            leaves = env.puct_begin(c=C / 256.0, max_tree_nodes=T, layout=layout, dtype=dtype)
            for i in range(sims + 1):
                if i in (0, 1, 5, sims):
                    other.set_state(leaves.boards, leaves.meta, leaves.legal)
                    want = other.observe(layout, dtype)
                    assert leaves.obs.dtype == dtype and leaves.obs.shape == want.shape
                    assert torch.equal(leaves.obs, want), (layout, dtype, i)
                if i < sims:
                    got = leaves_np(leaves)
                    priors, values = pf.hash_eval(got[1], got[2], n * n)
                    leaves = env.puct_advance(torch.from_numpy(priors).cuda(), torch.from_numpy(values).cuda(),
                                              more=i < sims - 1)
            assert int(leaves.kind.max()) == pf.NONE
    env.close()
    other.close()


def test_determinism_and_independence(torch_cuda):
    torch = torch_cuda
    c = pf.CASES[1]
    n, E, sims, C, T = c
    assert (n, E) == (6, 12)
    sims = 120
    s, run = pf.case(c)
    env = make_env(E, n)
    load(torch, env, s)
    a = hash_search(torch, env, n, sims, C, T)
    same_trace(a[0][:sims], run.leaves[:sims])
    # two runs give identical bytes
    b = hash_search(torch, env, n, sims, C, T)
    same_trace(b[0], a[0])
    same_outputs(b[1], a[1])
    # stepping the handle between begin and the advances changes nothing: the search keeps its root
    actions = torch.zeros(E, dtype=torch.int32, device="cuda:0")
    d = hash_search(torch, env, n, sims, C, T, between=lambda i: env.step(actions) if i in (0, 7) else None)
    same_trace(d[0], a[0], what="stepped")
    same_outputs(d[1], a[1], what="stepped")
    env.close()
    # boards 4..8 alone
    part = make_env(5, n)
    load(torch, part, subset(s, list(range(4, 9))))
    g = hash_search(torch, part, n, sims, C, T)
    same_trace(g[0], a[0], rows=slice(4, 9), what="boards 4..8")
    same_outputs(g[1], a[1], rows=slice(4, 9), what="boards 4..8")
    part.close()
    # any order of the boards: one handle a board
    for e in np.random.RandomState(5).permutation(E):
        one = make_env(1, n)
        load(torch, one, subset(s, [int(e)]))
        g = hash_search(torch, one, n, sims, C, T)
        same_trace(g[0], a[0], rows=slice(int(e), int(e) + 1), what="board %d" % e)
        same_outputs(g[1], a[1], rows=slice(int(e), int(e) + 1), what="board %d" % e)
        one.close()


def test_graph_replays_are_simulations(torch_cuda):
    """One advance captured with fixed uniform prior and value tensors, replayed S times, is S
    eager advances: the leaves after every replay and the outputs."""
    torch = torch_cuda
    S, E, n = 48, 9, 8
    env = make_env(E, n)
    env.reset()
    env.step_policy("random", 12, record=False)
    priors = torch.full((E, n * n), 4096, dtype=torch.int32, device="cuda:0")
    values = torch.zeros(E, dtype=torch.int32, device="cuda:0")
    kw = dict(c=1.25, max_tree_nodes=1024)
    leaves = env.puct_begin(**kw)
    eager = [[t.clone() for t in leaves]]
    for _ in range(S):
        leaves = env.puct_advance(priors, values)
        eager.append([t.clone() for t in leaves])
    want = env.puct_result(**ALL)
    ply = env.ply_counter
    leaves = env.puct_begin(**kw)  # the same workspace, warm
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # records only: the search has not moved
        out = env.puct_advance(priors, values)
    for x, y in zip(out, eager[0]):
        assert torch.equal(x, y)
    for i in range(S):
        g.replay()
        torch.cuda.synchronize()
        for name, x, y in zip(pf.LEAF_NAMES + ("obs",), out, eager[i + 1]):
            assert torch.equal(x, y), (name, i)
    for x, y in zip(env.puct_result(**ALL), want):
        assert torch.equal(x, y)
    assert int(want[0].sum(1).max()) == S - 1 and env.ply_counter == ply
    env.close()


def test_quantizer(torch_cuda):
    torch = torch_cuda
    from gymothelloenv_amd import puct_quantize
    E, n = 9, 8
    env = make_env(E, n, seed=4)
    env.reset()
    env.step_policy("random", 9, record=False)
    legal = env.get_state()[2]
    legal[3] = 0  # a row without a legal square
    mask = env.observe("legal", torch.int8).reshape(E, n * n).bool()
    mask[3] = False
    logits = torch.randn(E, n * n, device="cuda:0") * 3
    values = torch.tensor([1.0, -1.0, 0.25, 7.0, -7.0, 0.0, 0.5, -0.5, 1e-9], device="cuda:0")
    priors, vals = puct_quantize(logits, legal, values)
    assert priors.dtype == torch.int32 and vals.dtype == torch.int32 and priors.shape == (E, n * n)
    assert not priors[~mask].any() and int(priors.min()) >= 0 and int(priors.max()) <= 65535
    k = mask.sum(1)
    assert ((priors.sum(1) - 65535).abs() <= k)[k > 0].all() and not priors[3].any()  # each square rounds by <= 1/2
    assert vals.tolist() == [32768, -32768, 8192, 32768, -32768, 0, 16384, -16384, 0]
    # the softmax over the legal squares, in float32
    p = torch.softmax(logits.masked_fill(~mask, float("-inf")), 1)
    assert torch.equal(priors[k > 0], torch.round(p * 65535).to(torch.int32)[k > 0])
    env.close()


def test_search_loop_and_evaluators(torch_cuda):
    torch = torch_cuda
    import gymothelloenv_amd as g
    E, n, S = 9, 6, 24
    env = make_env(E, n, seed=2)
    env.reset()
    env.step_policy("random", 6, record=False)
    before = state_np(env)
    seen = []

    def net(leaves):  # any callable: here the uniform evaluator, watched
        assert leaves.obs.shape == (E, 4, n, n) and leaves.obs.dtype == torch.float32
        seen.append(leaves.kind.clone())
        return g.uniform_evaluator(leaves)

    vis, best, nodes, st = env.puct_search(net, S, best=True, tree_nodes=True, status=True)
    assert len(seen) == S and int(seen[0].min()) == pf.EXPAND
    assert (vis.sum(1) == S - 1).all() and (st == 0).all() and (nodes > 1).all()
    assert torch.equal(best, env.puct_actions(g.uniform_evaluator, S))
    assert (vis.gather(1, best.long()[:, None])[:, 0] == vis.max(1).values).all()
    # the loop by hand gives the same
    leaves = env.puct_begin(max_tree_nodes=S * (n * n - 4) // 4 + n * n)
    for i in range(S):
        logits, values = g.uniform_evaluator(leaves)
        pr, vl = g.puct_quantize(logits, leaves.legal, values)
        leaves = env.puct_advance(pr, vl, more=i < S - 1)
    assert torch.equal(env.puct_result(), vis)
    # the playout evaluator: a private env, seeded, so a search repeats
    a = env.puct_search(g.playout_evaluator(4, seed=9), S, value_sums=True)
    b = env.puct_search(g.playout_evaluator(4, seed=9), S, value_sums=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(a[1].any())
    for x, y in zip(before, state_np(env)):
        np.testing.assert_array_equal(x, y)
    with pytest.raises(ValueError, match="simulations"):
        env.puct_search(g.uniform_evaluator, 0)
    fresh = make_env(2, n)
    with pytest.raises(RuntimeError, match="puct_begin"):
        fresh.puct_result()
    fresh.close()
    env.close()


def test_argument_errors_on_a_live_handle(torch_cuda):
    from gymothelloenv_amd import OthelloLibError
    env = make_env(4, 8)
    env.reset()
    for kw, word in ((dict(c=-0.01), "c_puct"), (dict(c=256.5), "c_puct"), (dict(max_tree_nodes=63), "max_tree_nodes"),
                     (dict(max_tree_nodes=(1 << 24) + 1), "max_tree_nodes")):
        with pytest.raises(OthelloLibError, match=word):
            env.puct_begin(**kw)
    with pytest.raises(ValueError, match="layout"):
        env.puct_begin(layout="nope")
    env.close()


def test_puct_policy_replays_its_game(torch_cuda):
    import gymothelloenv_amd as g
    games = []
    for _ in range(2):
        opp = g.RandomPolicy(seed=1)
        env = g.OthelloEnv(white_policy=opp, black_policy=opp, protagonist=g.WHITE_DISK, board_size=6)
        pol = g.PUCTPolicy(simulations=24, seed=99)
        twin = g.playout_evaluator(8, seed=99)  # the policy's own evaluator, call for call
        moves = []
        with contextlib.redirect_stdout(io.StringIO()):
            obs = env.reset()
            pol.reset(env)
            done = False
            while not done:
                assert pol.counter == len(moves)
                legal = list(env.possible_moves)
                want = int(env.env._vec.puct_actions(twin, 24, c=1.25).cpu()[0])
                a = pol.get_action(obs)
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


def test_puct_beats_random_play(torch_cuda):
    """64 6x6 games as black against the device's random policy, one puct_search per move
    (64 simulations, the playout evaluator with 8 games a leaf): more wins than losses.  A
    sanity condition with a wide margin, not a strength measurement."""
    torch = torch_cuda
    import gymothelloenv_amd as g
    E, n = 64, 6
    env = make_env(E, n, seed=11)
    env.reset_vs("random", protagonist=-1)
    ev = g.playout_evaluator(8, seed=5)
    done = torch.zeros(E, dtype=torch.bool, device="cuda:0")
    for move in range(n * n):
        if bool(done.all()):
            break
        a = env.puct_actions(ev, 64)
        _, _, d, _ = env.step_vs(a, "random", observe=False)
        done |= d
    assert bool(done.all())
    discs = env.count_disks().cpu().numpy()  # (white, black)
    wins, losses = int((discs[:, 1] > discs[:, 0]).sum()), int((discs[:, 1] < discs[:, 0]).sum())
    print("PUCT (64 simulations, 8 playouts a leaf) as black against random on 64 6x6 boards: %d wins, %d losses" %
          (wins, losses))
    assert wins > losses
    env.close()
