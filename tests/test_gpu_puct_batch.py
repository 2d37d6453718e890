"""oth_puct_begin_batch / _advance_batch / _reroot_batch and their Python surface on
the device (K leaves a board per launch under virtual loss) against the plain
Python integers of tests/puct_batch_ref.py, the leaves compared after begin and
after every launch.  Every comparison with the reference is exact equality."""
import ctypes

import numpy as np
import pytest

import mcts_ref as mr
import puct_batch_ref as pb
import puct_play_ref as pp
import puct_ref as pf
from oracle import oracle

pytestmark = pytest.mark.gpu

ALL = dict(value_sums=True, best=True, tree_nodes=True, status=True)
VIEWS = (np.uint8, np.uint64, np.uint16, np.uint64)


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


def subset(s, rows):
    t = oracle.State(s.n, len(rows))
    t.boards[:], t.meta[:], t.legal[:] = s.boards[rows], s.meta[rows], s.legal[rows]
    return t


def leaves_np(leaves):
    return [t.cpu().numpy().view(v) for t, v in zip(leaves[:4], VIEWS)]


def outputs_np(env):
    return [t.cpu().numpy() for t in env.puct_result(**ALL)]


def hash_launch(torch, env, got, nn, sim_limit):
    priors, values = pf.hash_eval(got[1], got[2], nn)
    return leaves_np(env.puct_advance_batch(torch.from_numpy(priors).cuda(), torch.from_numpy(values).cuda(),
                                            sim_limit=sim_limit))


def hash_search(torch, env, n, sims, C, T, K, between=None, **begin):
    """The whole search with the reference's hash evaluator computed from the device's own leaves:
    launches with sim_limit = sims until no slot holds a leaf.  The trace and the outputs."""
    begin.setdefault("layout", None)
    trace = [leaves_np(env.puct_begin_batch(K, c=C / 256.0, max_tree_nodes=T, **begin))]
    while trace[-1][0].any():
        if between is not None:
            between(len(trace) - 1)
        trace.append(hash_launch(torch, env, trace[-1], n * n, sims))
        assert len(trace) <= sims + 2
    return trace, outputs_np(env)


def same_trace(got, want, rows=slice(None), what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        for name, x, y in zip(pf.LEAF_NAMES, g, w):
            np.testing.assert_array_equal(x, y[rows], err_msg="%s leaf %s after launch %d" % (what, name, i))


def same_outputs(got, want, rows=slice(None), what=""):
    for name, g, w in zip(pf.NAMES, got, want):
        np.testing.assert_array_equal(g, w[rows], err_msg="%s %s" % (what, name))


@pytest.mark.parametrize("c", pb.CASES, ids=lambda c: pb.CASE_ID % c)
def test_exact_against_the_reference(torch_cuda, c):
    torch = torch_cuda
    n, E, sims, C, T, K = c
    s, run = pb.case(c)
    pb.check_case(c, run)
    env = make_env(E, n, seed=3)
    load(torch, env, s)
    before = [t.clone() for t in env.get_state()]
    ply = env.ply_counter

    def between(i):  # result and pick between launches equal the reference's and change nothing
        if i in run.mid:
            ws = env._puct_ws.clone()
            same_outputs(outputs_np(env), run.mid[i][0], what="mid %d" % i)
            np.testing.assert_array_equal(env.puct_pick().cpu().numpy(), run.mid[i][1])
            assert torch.equal(env._puct_ws, ws)

    env._puct_ws = None
    need = ctypes.c_uint64(0)
    assert env._lib.oth_puct_batch_workspace_bytes(n, E, T, K, ctypes.byref(need)) == 0
    env._puct_ws = torch.full((need.value,), 0xA5, dtype=torch.uint8, device="cuda:0")  # a workspace of garbage
    trace, outs = hash_search(torch, env, n, sims, C, T, K, between=between)
    assert env._puct_ws.numel() == need.value
    same_trace(trace, run.leaves)
    same_outputs(outs, run.outputs)
    for x, y in zip(before, env.get_state()):  # nothing of the handle is written
        assert torch.equal(x, y)
    assert env.ply_counter == ply
    env.close()


@pytest.mark.parametrize("c", pb.K1_CASES, ids=lambda c: pf.CASE_ID % c)
def test_k1_is_the_plain_search(torch_cuda, c):
    """K = 1 against the plain calls themselves, launch by launch, and against puct_ref.Run."""
    torch = torch_cuda
    n, E, sims, C, T = c
    s = mr.positions(n, E)
    plain_ref = pf.Run(s.copy(), sims, C, T)
    env, twin = make_env(E, n), make_env(E, n)
    load(torch, env, s)
    load(torch, twin, s)
    lb = env.puct_begin_batch(1, c=C / 256.0, max_tree_nodes=T, layout="make_state")
    lp = twin.puct_begin(c=C / 256.0, max_tree_nodes=T, layout="make_state")
    for i in range(sims + 1):
        for name, x, y in zip(pf.LEAF_NAMES + ("obs",), lb, lp):
            assert torch.equal(x, y), (name, i)
        got = leaves_np(lb)
        for name, x, y in zip(pf.LEAF_NAMES, got, plain_ref.leaves[i]):
            np.testing.assert_array_equal(x, y, err_msg="%s %d" % (name, i))
        if i < sims:
            priors, values = pf.hash_eval(got[1], got[2], n * n)
            pr, vl = torch.from_numpy(priors).cuda(), torch.from_numpy(values).cuda()
            lb = env.puct_advance_batch(pr, vl, sim_limit=sims)
            lp = twin.puct_advance(pr, vl, more=i < sims - 1)
    for x, y in zip(env.puct_result(**ALL), twin.puct_result(**ALL)):
        assert torch.equal(x, y)
    same_outputs(outputs_np(env), plain_ref.outputs)
    env.close()
    twin.close()


@pytest.mark.parametrize("c", [pb.CASES[3], pb.CASES[6]], ids=lambda c: pb.CASE_ID % c)
def test_observation_of_the_leaves(torch_cuda, c):
    """obs is observe() of a second env of E K boards set_state'd to the leaf rows."""
    torch = torch_cuda
    n, E, sims, C, T, K = c
    assert (n, K) in ((8, 4), (10, 4))
    s, run = pb.case(c)
    env, other = make_env(E, n), make_env(E * K, n)
    load(torch, env, s)
    for layout, dtype in (("make_state", torch.float32), ("board", torch.int8)):
        leaves = env.puct_begin_batch(K, c=C / 256.0, max_tree_nodes=T, layout=layout, dtype=dtype)
        for i in range(7):
            other.set_state(leaves.boards, leaves.meta, leaves.legal)
            want = other.observe(layout, dtype)
            assert leaves.obs.dtype == dtype and leaves.obs.shape == want.shape and want.shape[0] == E * K
            assert torch.equal(leaves.obs, want), (layout, dtype, i)
            got = leaves_np(leaves)
            for name, x, y in zip(pf.LEAF_NAMES, got, run.leaves[i] if i <= 5 else ()):
                np.testing.assert_array_equal(x, y, err_msg=name)
            leaves = env.puct_advance_batch(*[torch.from_numpy(a).cuda() for a in pf.hash_eval(got[1], got[2], n * n)],
                                            sim_limit=sims if i < 5 else 0)
        assert not bool(leaves.kind.any())  # sim_limit = 0: nothing is selected
        other.set_state(leaves.boards, leaves.meta, leaves.legal)
        assert torch.equal(leaves.obs, other.observe(layout, dtype))
    env.close()
    other.close()


def test_determinism_and_independence(torch_cuda):
    torch = torch_cuda
    c = pb.CASES[8]
    n, E, sims, C, T, K = c
    assert E == 70
    s, run = pb.case(c)
    env = make_env(E, n)
    load(torch, env, s)
    a = hash_search(torch, env, n, sims, C, T, K)
    b = hash_search(torch, env, n, sims, C, T, K)  # two runs give identical bytes
    same_trace(b[0], a[0])
    same_outputs(b[1], a[1])
    env.close()
    for e in (0, 3, 37, 64, 69):  # a board alone: its own rows of the batch of 70, until its own search ends
        one = make_env(1, n)
        load(torch, one, subset(s, [e]))
        g = hash_search(torch, one, n, sims, C, T, K)
        rows = slice(e * K, (e + 1) * K)
        same_trace(g[0], a[0][:len(g[0])], rows=rows, what="board %d" % e)
        assert not any(t[0][rows].any() for t in a[0][len(g[0]):])
        same_outputs(g[1], a[1], rows=slice(e, e + 1), what="board %d" % e)
        one.close()


def test_graph_replays_are_launches(torch_cuda):
    """One advance_batch captured with fixed prior and value tensors, replayed, is that many launches."""
    torch = torch_cuda
    R, E, n, K = 10, 9, 8, 4
    env = make_env(E, n)
    env.reset()
    env.step_policy("random", 12, record=False)
    priors = torch.full((E * K, n * n), 4096, dtype=torch.int32, device="cuda:0")
    values = torch.zeros(E * K, dtype=torch.int32, device="cuda:0")
    kw = dict(c=1.25, max_tree_nodes=1024)
    leaves = env.puct_begin_batch(K, **kw)
    eager = [[t.clone() for t in leaves]]
    for _ in range(R):
        leaves = env.puct_advance_batch(priors, values)
        eager.append([t.clone() for t in leaves])
    want = env.puct_result(**ALL)
    leaves = env.puct_begin_batch(K, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # records only: the search has not moved
        out = env.puct_advance_batch(priors, values)
        with pytest.raises(RuntimeError, match="capture"):
            env.puct_search(None, 8, leaves_per_board=K)
    for x, y in zip(out, eager[0]):
        assert torch.equal(x, y)
    for i in range(R):
        g.replay()
        torch.cuda.synchronize()
        for name, x, y in zip(pf.LEAF_NAMES + ("obs",), out, eager[i + 1]):
            assert torch.equal(x, y), (name, i)
    for x, y in zip(env.puct_result(**ALL), want):
        assert torch.equal(x, y)
    assert int(want[0].sum(1).max()) > R  # more than one simulation a launch
    env.close()


def test_self_play_against_the_reference(torch_cuda):
    """9 boards, 8 x 8, K = 4, 2 moves of 30 simulations: launches, result, pick, step and reroot_batch with
    root priors, against puct_batch_ref.Game after every launch, with kept and tree_nodes."""
    torch = torch_cuda
    c = (8, 9, 30, 2, 320, 4096, 4)
    n, E, S, M, C, T, K = c
    s, g = pb.game(c)
    assert g.counters["kept"] > 0 and g.counters["fresh"] > 0 and g.counters["priors_set"] > 0
    assert g.moves[1]["launches"] == 3 and g.leaves[-2][0].any()  # leaves pending at the second re-root
    env = make_env(E, n, seed=pp.SEED)
    load(torch, env, s)
    it = iter(g.leaves)
    got = leaves_np(env.puct_begin_batch(K, c=C / 256.0, max_tree_nodes=T, layout=None))
    for name, x, y in zip(pf.LEAF_NAMES, got, next(it)):
        np.testing.assert_array_equal(x, y, err_msg=name)
    sample = torch.from_numpy(g.sample).cuda()
    for m, mv in enumerate(g.moves):
        for i in range(mv["launches"]):
            got = hash_launch(torch, env, got, n * n, mv["limit"])
            for name, x, y in zip(pf.LEAF_NAMES, got, next(it)):
                np.testing.assert_array_equal(x, y, err_msg="move %d launch %d %s" % (m, i, name))
        same_outputs(outputs_np(env), mv["results"], what="move %d" % m)
        picks = env.puct_pick(sample, seed=pp.SEED, counter=mv["counter"])
        np.testing.assert_array_equal(picks.cpu().numpy(), mv["picks"])
        acts = torch.from_numpy(mv["actions"]).cuda()
        env.step(acts, observe=False)
        rp = mv["root_priors"]
        leaves, kept = env.puct_reroot_batch(acts, None if rp is None else torch.from_numpy(rp).cuda(), kept=True,
                                             sim_limit=S * (m + 2))
        np.testing.assert_array_equal(kept.cpu().numpy(), mv["kept"])
        got = leaves_np(leaves)
        for name, x, y in zip(pf.LEAF_NAMES, got, next(it)):
            np.testing.assert_array_equal(x, y, err_msg="move %d reroot %s" % (m, name))
        np.testing.assert_array_equal(env.puct_result(tree_nodes=True)[1].cpu().numpy(), mv["used"])
    env.close()


def test_search_loop(torch_cuda):
    """puct_search(leaves_per_board=4) ends every DONE board at exactly `simulations`; with the uniform
    evaluator it equals the reference driven the same way (the integers puct_quantize makes of zeros)."""
    torch = torch_cuda
    import gymothelloenv_amd as g
    n, E, S, K = 8, 9, 50, 4
    s = mr.positions(n, E)
    env = make_env(E, n)
    load(torch, env, s)
    T = S * (n * n - 4) // 4 + n * n
    calls = []

    def net(leaves):
        assert leaves.obs.shape == (E * K, 4, n, n) and leaves.kind.shape == (E * K,)
        calls.append(int((leaves.kind != 0).sum()))
        return g.uniform_evaluator(leaves)

    vis, sums, best, nodes, st = env.puct_search(net, S, leaves_per_board=K, c=1.25, **ALL)
    done = (st == 0).cpu().numpy()
    assert done.sum() >= 3 and not done.all()
    # the root's simulations: one for the root alone, the others through its children
    assert (vis.sum(1).cpu().numpy()[done] == S - 1).all() and not vis.cpu().numpy()[~done].any()
    assert S // K <= len(calls) < S and max(calls) > E
    sr = pb.Search(s.copy(), 320, T, K)
    legal = pf.pr.legal_bool  # the uniform prior: round(65535 / k) on the leaf's squares
    while True:
        kind, boards, meta, lg = sr.leaves()
        if not kind.any():
            break
        mask = np.stack([legal(row, n * n) for row in lg])
        k = np.maximum(mask.sum(1, keepdims=True), 1)
        pri = np.where(mask, np.round(np.float32(65535) * (np.float32(1) / k.astype(np.float32))), 0).astype(np.int32)
        sr.advance(pri, np.zeros(E * K, dtype=np.int32), S)
    for name, a, b in zip(pf.NAMES, [t.cpu().numpy() for t in (vis, sums, best, nodes, st)], sr.result()):
        np.testing.assert_array_equal(a, b, err_msg=name)
    assert torch.equal(best, env.puct_actions(g.uniform_evaluator, S, leaves_per_board=K))
    env.close()
    # one move of self-play with the same keyword
    env = make_env(E, n)
    load(torch, env, s)
    play = env.puct_play(g.uniform_evaluator, 24, leaves_per_board=K)
    assert play.visits.shape == (E, n * n) and play.kept.shape == (E,) and bool(play.kept.any())
    assert (play.visits.sum(1).cpu().numpy()[done] == 23).all()
    with pytest.raises(RuntimeError, match="leaves_per_board"):
        env.puct_play(g.uniform_evaluator, 24)
    with pytest.raises(RuntimeError, match="began"):
        env.puct_advance(torch.zeros(E, n * n, dtype=torch.int32), torch.zeros(E, dtype=torch.int32))
    env.close()


def test_argument_errors_on_a_live_handle(torch_cuda):
    torch = torch_cuda
    from gymothelloenv_amd import OthelloLibError
    from gymothelloenv_amd import _lib as L
    E, n, K = 4, 8, 4
    env = make_env(E, n)
    env.reset()
    for k in (0, 65):
        with pytest.raises(ValueError, match="leaves_per_board"):
            env.puct_begin_batch(k)
    for kw, word in ((dict(c=-0.01), "c_puct"), (dict(max_tree_nodes=63), "max_tree_nodes")):
        with pytest.raises(OthelloLibError, match=word):
            env.puct_begin_batch(K, **kw)
    with pytest.raises(RuntimeError, match="puct_begin"):
        env.puct_advance_batch(None, None)
    leaves = env.puct_begin_batch(K, max_tree_nodes=256, layout=None)
    pr = torch.zeros(E * K, n * n, dtype=torch.int32, device="cuda:0")
    vl = torch.zeros(E * K, dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError, match="priors"):
        env.puct_advance_batch(pr[:E], vl)
    for lim in (-1, 1 << 24):
        with pytest.raises(ValueError, match="sim_limit"):
            env.puct_advance_batch(pr, vl, sim_limit=lim)
        with pytest.raises(ValueError, match="sim_limit"):
            env.puct_reroot_batch(torch.zeros(E, dtype=torch.int32), sim_limit=lim)
    # the C ABI on the live handle: K, sim_limit and the size, with nothing launched
    p, lv, _ = env._puct
    ws, kind = env._puct_ws, leaves.kind.clone()
    wsp, ptr = ctypes.c_void_p(ws.data_ptr()), lambda t: ctypes.c_void_p(t.data_ptr())
    need = ctypes.c_uint64(0)
    assert env._lib.oth_puct_batch_workspace_bytes(n, E, 256, K, ctypes.byref(need)) == 0
    bad = [(K, need.value, -1, b"sim_limit"), (K, need.value, 1 << 24, b"sim_limit"), (0, need.value, 5, b"K must"),
           (65, 1 << 40, 5, b"K must"), (K, need.value - 1, 5, b"oth_puct_batch_workspace_bytes")]
    for k, nbytes, lim, word in bad:
        rc = env._lib.oth_puct_advance_batch(env._h, ctypes.byref(p), k, wsp, nbytes, ptr(pr), ptr(vl), lim,
                                             ctypes.byref(lv), env._stream())
        assert rc == -1 and word in env._lib.oth_last_error(), (k, nbytes, lim)
    torch.cuda.synchronize()
    assert torch.equal(leaves.kind, kind)
    # another K on this workspace: the call is accepted and does nothing
    lt = torch.full((E * 2,), 7, dtype=torch.uint8, device="cuda:0")
    lv2 = L.OthPuctLeaves(lt.data_ptr(), None, None, None, None, 0, 0)
    before = ws.clone()
    assert env._lib.oth_puct_advance_batch(env._h, ctypes.byref(p), 2, wsp, ws.numel(), ptr(pr), ptr(vl), 5,
                                           ctypes.byref(lv2), env._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(ws, before) and bool((lt == 7).all())
    env.close()
