"""oth_play_search, oth_reset_vs_search and oth_step_vs_search on the device
(VecOthelloEnv.play_search, reset_vs / step_vs with a SearchConfig opponent).
The control flow is checked against the oracle through the greedy-equivalent
policy (play_search_ref.geq: its searched move is oracle.greedy's), the move
choice against the reference loops of tests/play_search_ref.py.  Every
comparison is exact equality."""
import ctypes

import numpy as np
import pytest

import family_cases as fc
import play_search_ref as pr
import search_ref as sh
import solve_ref as sr
from oracle import oracle
from test_search_host import searchlib  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

FLAG_SETS = {0: {}, 3: dict(sudden_death_on_invalid_move=True, num_disk_as_reward=True), 4: dict(auto_reset=True)}
PLIES = {4: 6, 6: 8, 8: 8, 10: 6, 16: 3}  # the move-choice run's plies per size
PLIES.update(fc.PLAY_PLIES)               # (the other sizes run from tests/test_gpu_family_sizes.py)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def make_env(E, n, flags=0, **kw):
    from gymothelloenv_amd import VecOthelloEnv
    base = dict(sudden_death_on_invalid_move=False, num_disk_as_reward=False, auto_reset=False)
    base.update(FLAG_SETS[flags])
    base.update(kw)
    return VecOthelloEnv(E, board_size=n, device="cuda:0", **base)


def config(cfg):
    from gymothelloenv_amd import SearchConfig
    return SearchConfig(depth=cfg.depth, weights=cfg.weights, mobility=cfg.mobility, terminal=cfg.terminal,
                        endgame_empties=cfg.endgame_empties, max_nodes=cfg.max_nodes)


def load(torch, env, s):
    env.set_state(torch.from_numpy(s.boards.view(np.int64)).cuda(), torch.from_numpy(s.meta.view(np.int16)).cuda(),
                  torch.from_numpy(s.legal.view(np.int64)).cuda())


def state_np(env):
    b, m, lg = env.get_state()
    return (b.cpu().numpy().view(np.uint64), m.cpu().numpy().view(np.uint16), lg.cpu().numpy().view(np.uint64))


def state_of(env):
    s = oracle.State(env.board_size, env.num_envs)
    s.boards[:], s.meta[:], s.legal[:] = state_np(env)
    return s


def assert_state(env, s, what=""):
    for name, g, w in zip(("boards", "meta", "legal"), state_np(env), (s.boards, s.meta, s.legal)):
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (name, what))


def outputs(res):
    return [t.cpu().numpy().view(np.uint8) if t.dtype.itemsize == 1 else t.cpu().numpy() for t in res]


# ------------------------------------------------------------ 1. control flow, play mode
@pytest.mark.parametrize("rand", [0, 6])
@pytest.mark.parametrize("flags", [0, 3, 4])
@pytest.mark.parametrize("n", [4, 6, 8, 10, 16])
def test_play_control_flow_is_the_oracles(torch_cuda, n, flags, rand):
    plies = min(2 * n * n // 3, 40) if n == 16 else 2 * n * n // 3
    geq = config(pr.geq(n))
    for E in (1, 9, 65):
        kw = dict(initial_rand_steps=rand, seed=11, env_id_base=1000)
        env, twin = make_env(E, n, flags, **kw), make_env(E, n, flags, **kw)
        s = state_of(env)
        ply0 = env.ply_counter
        got = outputs(env.play_search(geq, geq, plies, fallbacks=True))
        a, r, d, wdl = oracle.rollout(s, flags, 1, plies, seed=11, id_base=1000, ply0=ply0, initial_rand_steps=rand)
        for name, g, w in zip(("actions", "rewards", "dones"), got, (a, r, d)):
            assert g.shape == (plies, E)
            np.testing.assert_array_equal(g, w, err_msg="%s E=%d" % (name, E))
        assert not got[3].any()
        assert_state(env, s, "E=%d" % E)
        np.testing.assert_array_equal(env.counts().cpu().numpy(), wdl)
        for x, y in zip(twin.step_policy("greedy", plies), got):
            np.testing.assert_array_equal(outputs([x])[0], y)
        assert env.ply_counter == twin.ply_counter == ply0 + plies
        env.close()
        twin.close()


# ------------------------------------------------------------ 2. control flow, vs mode
@pytest.mark.parametrize("rand", [0, 6])
@pytest.mark.parametrize("flags", [0, 3, 4])
@pytest.mark.parametrize("who", ["white", "black", "mixed"])
@pytest.mark.parametrize("n", [4, 8, 10])
def test_vs_control_flow_is_the_oracles(torch_cuda, n, who, flags, rand):
    torch = torch_cuda
    E = 65
    prot = {"white": np.ones(E), "black": -np.ones(E), "mixed": np.where(np.arange(E) % 3 == 0, -1, 1)}[who]
    prot = prot.astype(np.int8)
    geq = config(pr.geq(n))
    env = make_env(E, n, flags, initial_rand_steps=rand, seed=7, env_id_base=300)
    env.ply_counter = 5
    env.reset_vs(geq, protagonist=torch.from_numpy(prot))
    s = oracle.reset_vs(n, E, flags, 1, 5, seed=7, id_base=300, initial_rand_steps=rand, prot=prot)
    assert_state(env, s, "after reset_vs")
    wdl, vs = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64)
    for c in range(12):
        call = env.ply_counter
        assert call == 6 + c
        acts = oracle.greedy(s)
        live = (s.meta & 2) == 0  # (a board terminated before the call reports done again and is no new game)
        _, r, d, plies, fb = env.step_vs(torch.from_numpy(acts).cuda(), geq, observe=False, fallbacks=True)
        orw, od, opl = oracle.step_vs(s, flags, 1, call, acts, seed=7, id_base=300, initial_rand_steps=rand,
                                      prot=prot, wdl=wdl)
        np.testing.assert_array_equal(r.cpu().numpy(), orw, err_msg="rewards of call %d" % c)
        np.testing.assert_array_equal(d.cpu().numpy().view(np.uint8), od, err_msg="dones of call %d" % c)
        np.testing.assert_array_equal(plies.cpu().numpy(), opl, err_msg="plies of call %d" % c)
        assert not fb.any()
        assert_state(env, s, "after call %d" % c)
        fin = live & (od != 0)
        vs += [int((fin & (orw > 0)).sum()), int((fin & (orw == 0)).sum()), int((fin & (orw < 0)).sum())]
    np.testing.assert_array_equal(env.counts().cpu().numpy(), wdl)
    np.testing.assert_array_equal(env.counts_vs().cpu().numpy(), vs)
    assert env.ply_counter == 18
    env.close()


# ------------------------------------------------------------ 3. move choice, play mode
_PLAY = {}


def play_reference(L, n):
    """(start state, (actions, rewards, dones, fallbacks), final state) of the
    reference self-play run of a size, computed once and never changed."""
    if n not in _PLAY:
        start = pr.recomputed(sh.batch(n, 74)[0])
        end = start.copy()
        A, R, D, F, held = pr.play(L, end, pr.black_policy(n), pr.white_policy(n), PLIES[n])
        # by the reference alone: the run holds what it is there to check
        assert held["fallbacks"] >= 5 and held["passes"] >= 5 and held["endgame"] >= 5, held
        assert held["terminated"] - int(((start.meta & 2) != 0).sum()) >= 5, held
        _PLAY[n] = (start, (A, R, D, F), end)
    start, out, end = _PLAY[n]
    return start.copy(), out, end


def dev_play(torch, s, black, white, plies, **kw):
    env = make_env(s.E, s.n, **kw)
    load(torch, env, s)
    got = outputs(env.play_search(black, white, plies, fallbacks=True))
    st = state_np(env)
    env.close()
    return got, st


@pytest.mark.parametrize("n", [4, 6, 8, 10, 16])
def test_play_moves_are_the_references(torch_cuda, searchlib, n):  # noqa: F811
    start, want, end = play_reference(searchlib, n)
    got, st = dev_play(torch_cuda, start, config(pr.black_policy(n)), config(pr.white_policy(n)), PLIES[n])
    for name, g, w in zip(("actions", "rewards", "dones", "fallbacks"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=name)
    for name, g, w in zip(("boards", "meta", "legal"), st, (end.boards, end.meta, end.legal)):
        np.testing.assert_array_equal(g, w, err_msg=name)


# ------------------------------------------------------------ 4. move choice, vs mode
@pytest.mark.parametrize("first", ["protagonist", "opponent"])
@pytest.mark.parametrize("n", [4, 6, 8, 10, 16])
def test_vs_moves_are_the_references(torch_cuda, searchlib, n, first):  # noqa: F811
    torch = torch_cuda
    s = pr.recomputed(sh.batch(n, 74)[0])
    mover = np.where(s.meta & 1, 1, -1).astype(np.int8)
    prot = mover if first == "protagonist" else (-mover).astype(np.int8)
    opp = pr.black_policy(n)
    ref = pr.vs_calls(searchlib, s.copy(), opp, prot, 4)
    assert sum(int(c[4].sum()) for c in ref) >= 1  # the opponent falls back somewhere
    env = make_env(s.E, n)
    load(torch, env, s)
    cfg = config(opp)
    for c, (acts, r, d, plies, fb, after) in enumerate(ref):
        _, gr, gd, gp, gf = env.step_vs(torch.from_numpy(acts).cuda(), cfg, protagonist=torch.from_numpy(prot),
                                        observe=False, fallbacks=True)
        for name, g, w in zip(("rewards", "dones", "plies", "fallbacks"), outputs((gr, gd, gp, gf)), (r, d, plies, fb)):
            np.testing.assert_array_equal(g, w, err_msg="%s of call %d" % (name, c))
        assert_state(env, after, "after call %d" % c)
    # the observation of a search call is observe()'s after it
    twin = make_env(s.E, n)
    load(torch, twin, ref[-1][5])
    load(torch, env, ref[-2][5])
    o = env.step_vs(torch.from_numpy(ref[-1][0]).cuda(), cfg, protagonist=torch.from_numpy(prot))[0]
    assert torch.equal(o, twin.get_observation())
    env.close()
    twin.close()


# ------------------------------------------------------------ 5. shapes
@pytest.mark.parametrize("E", [1, 7, 8, 9, 63, 64, 65])
def test_shapes_small(torch_cuda, searchlib, E):  # noqa: F811
    start, want, end = play_reference(searchlib, 8)
    idx = np.arange(9, 9 + E)
    got, st = dev_play(torch_cuda, sr.subset(start, idx), config(pr.black_policy(8)), config(pr.white_policy(8)),
                       PLIES[8])
    for name, g, w in zip(("actions", "rewards", "dones", "fallbacks"), got, want):
        np.testing.assert_array_equal(g, w[:, idx], err_msg=name)
    np.testing.assert_array_equal(st[0], end.boards[idx])
    np.testing.assert_array_equal(st[1], end.meta[idx])


def test_shapes_second_chunk(torch_cuda, searchlib):  # noqa: F811
    """Eight boards, one group, with more than 64 root moves together: the wave
    takes a second chunk of tasks."""
    cand = sr.late_positions(8, 300, [30, 32, 34, 36], seed=21)
    counts = sr.legal_rows(cand.legal, 64).sum(1) * ((cand.meta & 2) == 0)
    top = np.argsort(-counts, kind="stable")[:8]
    assert counts[top].sum() > 64
    group = sr.subset(cand, top)
    black, white = pr.black_policy(8), pr.white_policy(8)
    end = group.copy()
    A, R, D, F, _ = pr.play(searchlib, end, black, white, 2)
    got, st = dev_play(torch_cuda, group, config(black), config(white), 2)
    for name, g, w in zip(("actions", "rewards", "dones", "fallbacks"), got, (A, R, D, F)):
        np.testing.assert_array_equal(g, w, err_msg=name)
    np.testing.assert_array_equal(st[0], end.boards)


def test_shapes_sparse_and_permuted(torch_cuda, searchlib):  # noqa: F811
    """Two boards in three are terminated or finish early (one empty square), so
    whole groups have no task in some rounds while others do; a board's results
    are those of the same board alone and under a permutation."""
    start, _, _ = play_reference(searchlib, 8)
    black = pr.Cfg(2, sh.weight_sets(8)["default"][0], 2, 64, 6, 40)
    white = pr.white_policy(8)
    live = np.flatnonzero(((start.meta & 2) == 0) & (pr.empties(start) >= 8))
    short = np.flatnonzero(((start.meta & 2) == 0) & (pr.empties(start) == 1))
    assert len(live) >= 20 and len(short) >= 2
    end = start.copy()
    want = pr.play(searchlib, end, black, white, 4)[:4]
    E = 2500
    i = np.arange(E)
    src = np.where(i % 3 == 0, live[(i // 3) % len(live)], np.where(i % 3 == 1, 0, short[i % len(short)]))
    src[900:1300] = np.where(i[900:1300] % 2 == 0, 0, short[0])  # whole groups that are finished after one round
    assert (start.meta[0] & 2) != 0
    cb, cw = config(black), config(white)
    got, st = dev_play(torch_cuda, sr.subset(start, src), cb, cw, 4)
    for name, g, w in zip(("actions", "rewards", "dones", "fallbacks"), got, want):
        np.testing.assert_array_equal(g, w[:, src], err_msg=name)
    np.testing.assert_array_equal(st[0], end.boards[src])
    np.testing.assert_array_equal(st[1], end.meta[src])
    # alone, and permuted
    one, _ = dev_play(torch_cuda, sr.subset(start, live[3:4]), cb, cw, 4)
    for g, w in zip(one, want):
        np.testing.assert_array_equal(g[:, 0], w[:, live[3]])
    perm = np.random.RandomState(5).permutation(start.E)
    pg, pst = dev_play(torch_cuda, sr.subset(start, perm), cb, cw, 4)
    for g, w in zip(pg, want):
        np.testing.assert_array_equal(g, w[:, perm])
    np.testing.assert_array_equal(pst[0], end.boards[perm])


# ------------------------------------------------------------ 6. independence, repeatability, capture
def test_two_calls_give_identical_bytes(torch_cuda, searchlib):  # noqa: F811
    start, _, _ = play_reference(searchlib, 8)
    cb, cw = config(pr.black_policy(8)), config(pr.white_policy(8))
    a = dev_play(torch_cuda, start, cb, cw, 5, flags=4, initial_rand_steps=4, seed=3)
    b = dev_play(torch_cuda, start, cb, cw, 5, flags=4, initial_rand_steps=4, seed=3)
    for x, y in zip(a[0] + list(a[1]), b[0] + list(b[1])):
        assert x.tobytes() == y.tobytes()


def test_capture_in_a_graph_region(torch_cuda):
    """play_search(n_plies=3) captured inside graph_region: each replay from the
    restored state draws fresh opening moves from the region's counter range --
    replay r equals an eager twin's call at counter base + 3 r -- and the eager
    counters are untouched."""
    torch = torch_cuda
    E, n, K = 300, 8, 3
    cfg = config(pr.Cfg(2, sh.weight_sets(n)["default"][0], 1, 64, 0, 1 << 20))
    kw = dict(initial_rand_steps=6, seed=9)
    env, twin = make_env(E, n, 4, **kw), make_env(E, n, 4, **kw)
    twin.play_search(cfg, None, 1, record=False)  # (the config's device weights exist before the capture)
    env.reset()
    twin.reset()
    twin.ply_counter = 0
    sd = env.state_dict()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), env.graph_region() as slot:
        out = env.play_search(cfg, None, K, fallbacks=True)
    torch.cuda.synchronize()
    assert env.ply_counter == 0
    base = env.graph_counter_base(slot)
    prev = None
    for r in range(2):
        env.set_state(sd["boards"], sd["meta"], sd["legal"])
        twin.set_state(sd["boards"], sd["meta"], sd["legal"])
        twin.ply_counter = base + r * K
        graph.replay()
        torch.cuda.synchronize()
        want = twin.play_search(cfg, None, K, fallbacks=True)
        for x, y in zip(out, want):
            assert torch.equal(x, y)
        for x, y in zip(env.get_state(), twin.get_state()):
            assert torch.equal(x, y)
        if prev is not None:
            assert not torch.equal(prev, out[0])  # fresh opening moves per replay
        prev = out[0].clone()
    assert env.ply_counter == 0 and env.graph_offsets(slot)[0] == 2 * K and env.graph_offsets(0) == (0, 0)
    env.close()
    twin.close()


# ------------------------------------------------------------ 7. refusals
def test_refusals_touch_nothing(torch_cuda):
    torch = torch_cuda
    from gymothelloenv_amd import _lib as L
    from gymothelloenv_amd.vec_env import _ptr
    E, n = 37, 8
    env, twin = make_env(E, n, seed=3), make_env(E, n, seed=3)
    for v in (env, twin):
        v.step_policy("random", 7, record=False)
    lib, h, st = env._lib, env._h, env._stream()
    w = env._search_weights(None)

    def pol(weights=w.data_ptr(), depth=2, mob=0, term=64, end=0, nodes=100):
        return L.OthSearchPolicy(weights, depth, mob, term, end, nodes)

    good = pol()
    bad = [pol(weights=None), pol(depth=0), pol(depth=15), pol(mob=128), pol(mob=-128), pol(term=0), pol(term=32768),
           pol(end=-1), pol(end=15), pol(nodes=0), pol(nodes=2 ** 32)]
    a, r = torch.full((2, E), 77, dtype=torch.int32).cuda(), torch.full((2, E), 77, dtype=torch.int32).cuda()
    d, f = torch.full((2, E), 77, dtype=torch.uint8).cuda(), torch.full((2, E), 77, dtype=torch.uint8).cuda()
    p1, f1 = torch.full((E,), 77, dtype=torch.int32).cuda(), torch.full((E,), 77, dtype=torch.int32).cuda()
    acts = torch.zeros(E, dtype=torch.int32).cuda()
    g = ctypes.addressof(good)
    calls = []
    for b in bad:
        x = ctypes.addressof(b)
        calls += [lambda x=x: lib.oth_play_search(h, x, g, 2, _ptr(a), _ptr(r), _ptr(d), _ptr(f), st),
                  lambda x=x: lib.oth_play_search(h, g, x, 2, _ptr(a), _ptr(r), _ptr(d), _ptr(f), st),
                  lambda x=x: lib.oth_reset_vs_search(h, x, None, None, st),
                  lambda x=x: lib.oth_step_vs_search(h, x, _ptr(acts), None, _ptr(r), _ptr(d), _ptr(p1), _ptr(f1), st)]
    calls += [lambda: lib.oth_play_search(None, g, g, 2, _ptr(a), _ptr(r), _ptr(d), _ptr(f), st),
              lambda: lib.oth_play_search(h, None, g, 2, _ptr(a), _ptr(r), _ptr(d), _ptr(f), st),
              lambda: lib.oth_play_search(h, g, None, 2, _ptr(a), _ptr(r), _ptr(d), _ptr(f), st),
              lambda: lib.oth_play_search(h, g, g, 0, _ptr(a), _ptr(r), _ptr(d), _ptr(f), st),
              lambda: lib.oth_play_search(h, g, g, -1, _ptr(a), _ptr(r), _ptr(d), _ptr(f), st),
              lambda: lib.oth_reset_vs_search(None, g, None, None, st),
              lambda: lib.oth_reset_vs_search(h, None, None, None, st),
              lambda: lib.oth_step_vs_search(None, g, _ptr(acts), None, _ptr(r), _ptr(d), _ptr(p1), _ptr(f1), st),
              lambda: lib.oth_step_vs_search(h, None, _ptr(acts), None, _ptr(r), _ptr(d), _ptr(p1), _ptr(f1), st),
              lambda: lib.oth_step_vs_search(h, g, None, None, _ptr(r), _ptr(d), _ptr(p1), _ptr(f1), st)]
    before, ply = state_np(env), env.ply_counter
    for k, call in enumerate(calls):
        assert call() == -1, k  # OTH_EINVAL
        assert lib.oth_last_error()
    torch.cuda.synchronize()
    for t in (a, r, d, f, p1, f1):
        assert (t == 77).all()
    for x, y in zip(before, state_np(env)):
        np.testing.assert_array_equal(x, y)
    assert env.ply_counter == ply == twin.ply_counter
    # the Python layer: wrong types, and a string opponent still takes the old path
    from gymothelloenv_amd import SearchConfig
    with pytest.raises(TypeError):
        env.play_search("greedy")
    with pytest.raises(ValueError):
        env.play_search(SearchConfig(depth=1), n_plies=0)
    with pytest.raises(ValueError):
        env.play_search(SearchConfig(weights=np.zeros(36, dtype=np.int8)))  # another board size's table
    with pytest.raises(ValueError):
        env.step_vs(acts, "greedy", fallbacks=True)
    for v in (env, twin):
        v.reset_vs("greedy")
    for x, y in zip(env.step_vs(env.greedy_actions(), "greedy"), twin.step_vs(twin.greedy_actions(), "greedy")):
        assert torch.equal(x, y)
    for x, y in zip(state_np(env), state_np(twin)):
        np.testing.assert_array_equal(x, y)
    assert env.ply_counter == twin.ply_counter == ply + 2
    env.close()
    twin.close()
