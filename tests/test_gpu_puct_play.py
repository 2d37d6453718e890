"""oth_puct_pick, oth_puct_reroot and VecOthelloEnv.puct_pick / puct_reroot / puct_play
on the device against the plain Python integers of tests/puct_play_ref.py (whole
games of begin, advances, pick, oth_step, reroot), every leaf and every output
compared after every call, in both mappings of the re-root's sweep: the shipped
library (a wave per board) and the second library with the whole call on one
lane (gymothelloenv_amd/variants/liboth_reroot_lane.so, -DOTH_PUCT_REROOT_LANE=1).
Every comparison with the reference is exact equality."""
import ctypes

import numpy as np
import pytest

import puct_play_ref as pp
import puct_ref as pf
from test_gpu_puct import ALL, leaves_np, load, make_env, same_outputs, state_np, subset, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lane_lib(torch_cuda):
    """The library whose oth_puct_reroot runs on one lane a board."""
    from gymothelloenv_amd import _lib as L
    from gymothelloenv_amd import build as hb
    if hb.needs_build(hb.REROOT_LANE_OUT, hb.REROOT_LANE_FLAGS):
        hb.build_reroot_lane(verbose=False)
    return L.load_path(hb.REROOT_LANE_OUT)


def same_leaves(got, want, what, rows=slice(None)):
    for name, g, w in zip(pf.LEAF_NAMES, got, want):
        np.testing.assert_array_equal(g, w[rows], err_msg="%s leaf %s" % (what, name))


def dev(torch, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def advances(torch, env, n, S, leaves, trace=None, last_more=True):
    for i in range(S):
        got = leaves_np(leaves)
        priors, values = pf.hash_eval(got[1], got[2], n * n)
        leaves = env.puct_advance(dev(torch, priors), dev(torch, values), more=last_more or i < S - 1)
        if trace is not None:
            trace.append(leaves_np(leaves))
    return leaves


def play(torch, env, game, c, rows=slice(None), id_key=pp.ID_KEY, what=""):
    """The reference's game on env (holding the boards `rows` of the case), everything compared
    after every call; returns the trace of the leaves."""
    n, E, S, M, C, T = c
    it = iter(game.leaves)
    leaves = env.puct_begin(c=C / 256.0, max_tree_nodes=T, layout=None)
    trace = [leaves_np(leaves)]
    same_leaves(trace[-1], next(it), what + "begin", rows)
    sample = dev(torch, game.sample[rows])
    for m, mv in enumerate(game.moves):
        for i in range(S):
            leaves = advances(torch, env, n, 1, leaves, trace)
            same_leaves(trace[-1], next(it), "%smove %d advance %d" % (what, m, i), rows)
        same_outputs([t.cpu().numpy() for t in env.puct_result(**ALL)], mv["results"], rows, "%smove %d" % (what, m))
        picks = env.puct_pick(sample, seed=pp.SEED, counter=mv["counter"]) if id_key == 0 else \
            raw_pick(torch, env, sample, pp.SEED, id_key, mv["counter"])
        np.testing.assert_array_equal(picks.cpu().numpy(), mv["picks"][rows], err_msg="%smove %d picks" % (what, m))
        _, rewards, dones, _ = env.step(dev(torch, mv["actions"][rows]), observe=False)
        np.testing.assert_array_equal(rewards.cpu().numpy(), mv["rewards"][rows])
        np.testing.assert_array_equal(dones.cpu().numpy().astype(np.uint8), mv["dones"][rows])
        st = mv["state"]
        for x, y in zip(state_np(env), (st.boards, st.meta, st.legal)):
            np.testing.assert_array_equal(x, y[rows], err_msg="%smove %d: the stepped handle" % (what, m))
        rp = mv["root_priors"]
        leaves, kept = env.puct_reroot(dev(torch, mv["actions"][rows]), None if rp is None else dev(torch, rp[rows]),
                                       kept=True)
        for x, y in zip(state_np(env), (st.boards, st.meta, st.legal)):
            np.testing.assert_array_equal(x, y[rows], err_msg="%smove %d: reroot wrote the handle" % (what, m))
        np.testing.assert_array_equal(kept.cpu().numpy(), mv["kept"][rows], err_msg="%smove %d kept" % (what, m))
        trace.append(leaves_np(leaves))
        same_leaves(trace[-1], next(it), "%smove %d reroot" % (what, m), rows)
        np.testing.assert_array_equal(env.puct_result(tree_nodes=True)[1].cpu().numpy(), mv["used"][rows],
                                      err_msg="%smove %d tree_nodes" % (what, m))
    return trace


def raw_pick(torch, env, sample, seed, id_key, counter):
    """oth_puct_pick through the C ABI (VecOthelloEnv.puct_pick passes id_key 0)."""
    from gymothelloenv_amd import _lib as L
    p, lv, leaves = env._puct
    out = torch.full((env.num_envs,), 77, dtype=torch.int32, device="cuda:0")
    L.check(env._lib.oth_puct_pick(env._h, ctypes.byref(p), ctypes.c_void_p(env._puct_ws.data_ptr()),
                                   env._puct_ws.numel(), None if sample is None else ctypes.c_void_p(sample.data_ptr()),
                                   seed, id_key, counter, ctypes.c_void_p(out.data_ptr()), env._stream()),
            "oth_puct_pick", env._lib)
    return out


@pytest.mark.parametrize("mapping", ["wave", "lane"])
@pytest.mark.parametrize("c", pp.CASES, ids=lambda c: pp.CASE_ID % c)
def test_exact_against_the_reference(torch_cuda, lane_lib, c, mapping):
    torch = torch_cuda
    n, E, S, M, C, T = c
    s, game = pp.case(c)
    pp.check_case(c, game)
    env = make_env(E, n, seed=3, **(dict(lib=lane_lib) if mapping == "lane" else {}))
    load(torch, env, s)
    # the workspace starts as garbage
    env.puct_begin(c=C / 256.0, max_tree_nodes=T, layout=None)
    env._puct_ws.fill_(0xA5)
    play(torch, env, game, c)
    env.close()


def test_the_in_place_sweep_beyond_the_table(torch_cuda):
    """A kept subtree of more slots than the wave sweep's table in LDS holds (4,096) goes in place
    on one lane: 8 x 8 boards after 800 simulations in trees of 8,192 slots."""
    torch = torch_cuda
    c = (8, 4, 800, 1, 320, 8192)
    n, E, S, M, C, T = c
    s = pp.mr.positions(n, E)
    game = pp.Game(s, S, M, C, T)
    mv = game.moves[0]
    assert ((mv["results"][3] > 4096 + 64) & (mv["kept"] == 1)).any(), "no kept board beyond the table"
    env = make_env(E, n)
    load(torch, env, s)
    leaves = env.puct_begin(c=C / 256.0, max_tree_nodes=T, layout=None)
    leaves = advances(torch, env, n, S, leaves)
    same_leaves(leaves_np(leaves), game.leaves[S], "before the reroot")
    env.step(dev(torch, mv["actions"]), observe=False)
    leaves, kept = env.puct_reroot(dev(torch, mv["actions"]), kept=True)
    np.testing.assert_array_equal(kept.cpu().numpy(), mv["kept"])
    same_leaves(leaves_np(leaves), game.leaves[S + 1], "reroot")
    np.testing.assert_array_equal(env.puct_result(tree_nodes=True)[1].cpu().numpy(), mv["used"])
    # the kept trees are whole: the search goes on as the reference's does
    ref = game.boards
    for i in range(20):
        got = leaves_np(leaves)
        priors, values = pf.hash_eval(got[1], got[2], n * n)
        for e, b in enumerate(ref):
            b.advance(priors[e], values[e], True)
        leaves = env.puct_advance(dev(torch, priors), dev(torch, values))
        same_leaves(leaves_np(leaves), game._leaves(), "advance %d after the reroot" % i)
    env.close()


@pytest.mark.parametrize("how", ["minus_one", "set_state"])
def test_reroot_elsewhere_is_begin(torch_cuda, how):
    """All actions -1, or a handle set_state'd to other positions: afterwards the search equals a
    fresh puct_begin on that handle state, leaves and results, through S more advances."""
    torch = torch_cuda
    c = pp.CASES[1]
    n, E, S, M, C, T = c
    s, game = pp.case(c)
    env = make_env(E, n)
    load(torch, env, s)
    leaves = advances(torch, env, n, S, env.puct_begin(c=C / 256.0, max_tree_nodes=T, layout=None))
    if how == "minus_one":
        actions, h = np.full(E, -1, dtype=np.int32), s
    else:
        actions, h = game.moves[0]["actions"], game.moves[3]["state"]  # three moves further on
        load(torch, env, h)
    leaves, kept = env.puct_reroot(dev(torch, actions), kept=True)
    assert not kept.any()
    got = [leaves_np(leaves)]
    advances(torch, env, n, S, leaves, got)
    outs = [t.cpu().numpy() for t in env.puct_result(**ALL)]
    fresh = make_env(E, n)
    load(torch, fresh, h)
    want = [leaves_np(fresh.puct_begin(c=C / 256.0, max_tree_nodes=T, layout=None))]
    advances(torch, fresh, n, S, fresh._puct[2], want)
    for i, (g, w) in enumerate(zip(got, want)):
        same_leaves(g, w, "launch %d" % i)
    same_outputs(outs, [t.cpu().numpy() for t in fresh.puct_result(**ALL)])
    assert (outs[4] == pf.DONE).any() and outs[0].any()
    env.close()
    fresh.close()


def test_determinism_and_independence(torch_cuda):
    torch = torch_cuda
    c = pp.CASES[1]
    n, E, S, M, C, T = c
    assert (n, E) == (6, 12)
    c = (n, E, S, 5, C, T)
    s, _ = pp.case(pp.CASES[1])
    game = pp.Game(s, S, 5, C, T)
    env = make_env(E, n)
    load(torch, env, s)
    a = play(torch, env, game, c)
    # two runs give identical bytes
    load(torch, env, s)
    b = play(torch, env, game, c)
    for x, y in zip(a, b):
        same_leaves(x, y, "second run")
    env.close()
    # a sentinel past workspace_bytes is untouched (the C ABI on a workspace of the exact size)
    from gymothelloenv_amd import _lib as L
    env = make_env(E, n)
    load(torch, env, s)
    need = ctypes.c_uint64(0)
    L.check(env._lib.oth_puct_workspace_bytes(n, E, T, ctypes.byref(need)))
    big = torch.full((need.value + 4096,), 0x5C, dtype=torch.uint8, device="cuda:0")

    class Exact(object):  # the tensor with the exact size reported to the library
        def __init__(self, t):
            self.t = t

        def numel(self):
            return need.value

        def data_ptr(self):
            return self.t.data_ptr()

        def fill_(self, v):
            return self.t.fill_(v)

    env._puct_ws = Exact(big)
    play(torch, env, game, c)
    assert isinstance(env._puct_ws, Exact) and bool((big[need.value:] == 0x5C).all())
    assert not bool((big[:need.value] == 0x5C).all())
    env._puct_ws = None
    env.close()
    # boards 4..8 alone, as a shard with env_id_base = 4: the same traces, the same sampled moves
    part = make_env(5, n, env_id_base=4)
    load(torch, part, subset(s, list(range(4, 9))))
    play(torch, part, game, c, rows=slice(4, 9), what="boards 4..8 ")
    part.close()
    # any board alone at index 0, next to no neighbours
    for e in (0, 4, 7, 11):
        one = make_env(1, n, env_id_base=e)
        load(torch, one, subset(s, [e]))
        play(torch, one, game, c, rows=slice(e, e + 1), what="board %d " % e)
        one.close()


def test_root_priors(torch_cuda):
    """Children of kept roots take the clamped values (seen through the selection: the reference
    agrees on every later leaf); NULL leaves them; fresh roots ignore them."""
    torch = torch_cuda
    c = pp.CASES[1]
    n, E, S, M, C, T = c
    s, _ = pp.case(c)
    nn = n * n
    rs = np.random.RandomState(7)
    table = rs.randint(-70000, 140000, size=(E, nn)).astype(np.int32)  # far outside [0, 65535] on both sides

    def run(priors):
        game = pp.Game(s, S, 3, C, T, priors=priors)
        env = make_env(E, n)
        load(torch, env, s)
        trace = play(torch, env, game, (n, E, S, 3, C, T))
        env.close()
        return game, trace

    with_p, tr_p = run(lambda cur, m: table)
    without, tr_n = run(None)
    assert with_p.counters["priors_set"] > 0 and without.counters["priors_set"] == 0
    differ = [i for i, (x, y) in enumerate(zip(tr_p, tr_n)) if any((a != b).any() for a, b in zip(x, y))]
    assert differ and differ[0] >= S + 1, "the priors steer the selection, from the first re-root on"
    # a board that begins afresh at the re-root ignores them: its trace is the one without priors
    fresh = np.flatnonzero(with_p.moves[0]["kept"] == 0)
    assert fresh.size
    for x, y in zip(tr_p[:2 * (S + 1)], tr_n[:2 * (S + 1)]):
        for a, b in zip(x, y):
            np.testing.assert_array_equal(a[fresh], b[fresh])


@pytest.mark.parametrize("c", [pp.CASES[3], pp.CASES[4]], ids=lambda c: pp.CASE_ID % c)
def test_observation_after_reroot(torch_cuda, c):
    """obs after reroot is observe() of a handle set_state'd to the leaf arrays."""
    torch = torch_cuda
    n, E, S, M, C, T = c
    assert n in (8, 10)
    s, game = pp.case(c)
    mv = game.moves[0]
    env, other = make_env(E, n), make_env(E, n)
    for layout, dtype in (("make_state", torch.float32), ("board_legal", torch.int8), ("absolute", torch.bfloat16)):
        load(torch, env, s)
        leaves = env.puct_begin(c=C / 256.0, max_tree_nodes=T, layout=layout, dtype=dtype)
        leaves = advances(torch, env, n, 12, leaves)
        picks = env.puct_pick()
        env.step(picks, observe=False)
        leaves, kept = env.puct_reroot(picks, kept=True)
        assert bool(kept.any()) and not bool(kept.all())
        other.set_state(leaves.boards, leaves.meta, leaves.legal)
        want = other.observe(layout, dtype)
        assert leaves.obs.dtype == dtype and leaves.obs.shape == want.shape and torch.equal(leaves.obs, want)
    env.close()
    other.close()


def test_sampling(torch_cuda):
    """pick with sample on is the reference's Philox draw, a sharded handle gives the matching
    slice, sample off is puct_result's best."""
    torch = torch_cuda
    c = pp.CASES[1]
    n, E, S, M, C, T = c
    s, _ = pp.case(c)
    seed, counter = 0xFEDCBA9876543210, 2 ** 63 + 11
    ref = pf.Search(s, C, T)
    ref.boards = [pp.Board(s, e, C, T, dict((k, 0) for k in pf.COUNTERS + pp.COUNTERS)) for e in range(E)]
    env, shard = make_env(E, n, env_id_base=2 ** 32 - 5), make_env(5, n, env_id_base=2 ** 32 - 1)
    load(torch, env, s)
    load(torch, shard, subset(s, list(range(4, 9))))
    leaves, sl = env.puct_begin(c=C / 256.0, max_tree_nodes=T, layout=None), \
        shard.puct_begin(c=C / 256.0, max_tree_nodes=T, layout=None)
    for i in range(S):
        got = leaves_np(leaves)
        priors, values = pf.hash_eval(got[1], got[2], n * n)
        ref.advance(priors, values, True)
        leaves = env.puct_advance(dev(torch, priors), dev(torch, values))
        sl = shard.puct_advance(dev(torch, priors[4:9]), dev(torch, values[4:9]))
    best = env.puct_result(best=True)[1]
    assert torch.equal(env.puct_pick(), best) and torch.equal(env.puct_pick(sample=torch.zeros(E)), best)
    seen_other = False
    for k in range(6):
        want = np.array([b.pick(True, seed, (2 ** 32 - 5 + e) % 2 ** 32, counter + k) for e, b in enumerate(ref.boards)],
                        dtype=np.int32)
        got = env.puct_pick(True, seed=seed, counter=counter + k)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        np.testing.assert_array_equal(shard.puct_pick(True, seed=seed, counter=counter + k).cpu().numpy(), want[4:9])
        seen_other |= bool((got != best).any())
    assert seen_other and (want[[0, 2, 3]] >= 0).all() and want[1] == -1
    # the counter of its own: it moves on with every call that passes a sample and gives no counter
    assert env.puct_pick_counter == 1  # (the call with a sample of zeros above)
    a = env.puct_pick(True)
    env.puct_pick()
    env.puct_pick(True, counter=77)
    assert env.puct_pick_counter == 2
    env.puct_pick_counter = 1
    assert torch.equal(env.puct_pick(True), a)
    env.close()
    shard.close()


def test_graph_of_pick_step_reroot(torch_cuda):
    """One capture of pick -> oth_step -> reroot, replayed once, equals the eager calls."""
    torch = torch_cuda
    S, E, n = 24, 9, 8
    kw = dict(c=1.25, max_tree_nodes=1024, layout="make_state")
    priors = torch.full((E, n * n), 4096, dtype=torch.int32, device="cuda:0")
    values = torch.zeros(E, dtype=torch.int32, device="cuda:0")
    sample = (torch.arange(E, device="cuda:0") % 2).to(torch.uint8)

    def prepare():
        env = make_env(E, n, seed=5)
        env.reset()
        env.step_policy("random", 12, record=False)
        env.puct_begin(**kw)
        for _ in range(S):
            env.puct_advance(priors, values)
        return env

    def move(env):
        a = env.puct_pick(sample, counter=3)
        _, r, d, _ = env.step(a, observe=False)
        leaves, kept = env.puct_reroot(a, kept=True)
        return [a, r, d, kept] + list(leaves)

    eager_env = prepare()
    eager = [t.clone() for t in move(eager_env)]
    eager_state = state_np(eager_env)
    eager_vis = eager_env.puct_result(tree_nodes=True)
    env = prepare()
    before = state_np(env)
    ws = env._puct_ws.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # records only
        out = move(env)
    for x, y in zip(state_np(env), before):
        np.testing.assert_array_equal(x, y)
    assert torch.equal(env._puct_ws, ws)
    g.replay()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(out, eager)):
        assert torch.equal(x, y), i
    for x, y in zip(state_np(env), eager_state):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(env.puct_result(tree_nodes=True), eager_vis):
        assert torch.equal(x, y)
    assert bool(eager[3].any())
    env.close()
    eager_env.close()


def test_puct_play(torch_cuda):
    """puct_play with the uniform evaluator on 64 6 x 6 boards: every game reaches its end, a kept
    board's next search starts above S - 1 visits, and with auto-reset the loop goes on."""
    torch = torch_cuda
    import gymothelloenv_amd as g
    E, n, S = 64, 6, 16
    env = make_env(E, n, seed=7)
    env.reset()
    done = torch.zeros(E, dtype=torch.bool, device="cuda:0")
    kept_before, reused = torch.zeros(E, dtype=torch.bool, device="cuda:0"), 0
    for move in range(n * n):
        out = env.puct_play(g.uniform_evaluator, S, sample=move < 6)
        assert isinstance(out, g.PuctPlay) and out.visits.shape == (E, n * n) and out.kept.dtype == torch.uint8
        total = out.visits.sum(1)
        assert bool((total[kept_before] > S - 1).all()), "a kept tree brings its visits along"
        assert bool((total[~kept_before & ~done] == S - 1).all()) and not bool(total[done].any())
        assert bool((out.actions[done] == -1).all()) and bool((out.actions[~done] >= 0).all())
        played = out.visits.gather(1, out.actions.clamp(min=0).long()[:, None])[:, 0]
        assert bool((played[~done] > 0).all()), "the move is a visited child"
        reused += int(kept_before.sum())
        done |= out.dones
        assert not bool((out.kept.bool() & done).any())
        kept_before = out.kept.bool()
        if bool(done.all()):
            break
    assert bool(done.all()) and reused > E
    assert env.puct_pick_counter == min(move + 1, 6)
    env.close()
    # auto-reset: the loop keeps going past a game end, the reset boards begin afresh
    env = make_env(8, 4, seed=1, auto_reset=True)
    env.reset()
    ends = 0
    for move in range(40):
        out = env.puct_play(g.uniform_evaluator, 8)
        ends += int(out.dones.sum())
        assert bool((out.actions >= 0).all())
    assert ends > 8
    env.close()
