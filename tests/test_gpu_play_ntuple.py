"""oth_play_ntuple, oth_reset_vs_ntuple, oth_step_vs_ntuple and oth_ntuple_update_masked on
the device (VecOthelloEnv.play_ntuple, reset_vs / step_vs with an NTuplePlayer opponent,
NTupleNet.update(mask=...), NTupleNet.td_play).  The control flow is checked against the
oracle through the greedy-equivalent policy (play_ntuple_ref.geq: its move is
oracle.greedy's), the move choice, the exploring draws and the TD rows against the
reference loops of tests/play_ntuple_ref.py.  Every comparison is exact equality."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

import ntuple_cases as nc
import ntuple_ref as nr
import play_ntuple_ref as pn
import play_search_ref as pr
import rng_ref as rr
import search_ref as sh
import solve_ref as sr
from oracle import oracle

pytestmark = pytest.mark.gpu

FLAG_SETS = {0: {}, 3: dict(sudden_death_on_invalid_move=True, num_disk_as_reward=True), 4: dict(auto_reset=True)}
PLIES = {4: 6, 6: 8, 8: 8, 10: 6, 16: 3}  # the move-choice run's plies per size, as tests/test_gpu_play_search.py's
NAMES = ("actions", "rewards", "dones", "fallbacks")
TD_NAMES = ("td boards", "td meta", "td targets", "td learn")


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


def make_net(torch, n, tp, shift, weights=None):
    import gymothelloenv_amd as g
    net = g.NTupleNet(n, tp, shift, device="cuda:0")
    if weights is not None:
        net.weights.copy_(torch.from_numpy(np.ascontiguousarray(weights, dtype=np.int32)))
    return net


def player(torch, n, p):
    """The NTuplePlayer of a reference policy."""
    import gymothelloenv_amd as g
    pl = g.NTuplePlayer(make_net(torch, n, p.tuples, p.shift, p.weights), depth=p.depth,
                        endgame_empties=p.endgame_empties, explore=p.explore / 65536.0, terminal=p.terminal,
                        max_nodes=p.max_nodes)
    assert pl.explore == p.explore
    return pl


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


def host(t):
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int64): np.uint64, np.dtype(np.int16): np.uint16, np.dtype(bool): np.uint8}.get(a.dtype, a.dtype))


def outputs(res):
    """A play_ntuple result as numpy arrays: the four outputs, then the four td arrays if any."""
    flat = []
    for t in res:
        flat += [host(x) for x in t] if isinstance(t, tuple) else [host(t)]
    return flat


def policies(n):
    """Black's and white's policy of the move-choice runs: two different nets, depth 2 under a budget of 6
    placements a root move and endgame mode from 4 empty squares against depth 1."""
    tb, sb, wb = nc.search_net(n)
    cw = nc.case(n, 32, "mixed")
    return (pn.pol(tb, sb, wb, depth=2, terminal=64, endgame_empties=4, max_nodes=6),
            pn.pol(cw.tuples, 9, cw.weights, depth=1, terminal=1000))


_PLAY = {}


def play_reference(n):
    """(start state, the Run, final state) of the reference self-play run of a size (flags 0), computed once
    and never changed."""
    if n not in _PLAY:
        start = pr.recomputed(sh.batch(n, 74)[0])
        end = start.copy()
        run = pn.play(end, *policies(n), PLIES[n])
        h = run.held  # by the reference alone: the run holds what it is there to check
        assert h["fallbacks"] >= 1 and h["passes"] >= 1 and h["endgame"] >= 1, dict(h)
        assert h["terminated"] - int(((start.meta & 2) != 0).sum()) >= 5, dict(h)
        _PLAY[n] = (start, run, end)
    start, run, end = _PLAY[n]
    return start.copy(), run, end


def dev_play(torch, s, black, white, plies, td=False, flags=0, **kw):
    """play_ntuple on State s: (the outputs and td arrays as numpy, the state after, the counts)."""
    env = make_env(s.E, s.n, flags, **kw)
    load(torch, env, s)
    pb = player(torch, s.n, black)
    pw = pb if white is black else player(torch, s.n, white)
    got = outputs(env.play_ntuple(pb, pw, plies, fallbacks=True, td=td))
    st, counts = state_np(env), env.counts().cpu().numpy()
    env.close()
    return got, st, counts


def want_of(run, td=False):
    return [run.actions, run.rewards, run.dones, run.fallbacks] + ([run.boards, run.meta, run.targets, run.learn] if td else [])


# ------------------------------------------------------------ 1. moves and outputs against the reference
@pytest.mark.parametrize("n", [4, 6, 8, 10, 16])
def test_play_moves_are_the_references(torch_cuda, n):
    start, run, end = play_reference(n)
    got, st, _ = dev_play(torch_cuda, start, *policies(n), PLIES[n])
    for name, g, w in zip(NAMES, got, want_of(run)):
        assert g.shape == (PLIES[n], 74)
        np.testing.assert_array_equal(g, w, err_msg=name)
    for name, g, w in zip(("boards", "meta", "legal"), st, (end.boards, end.meta, end.legal)):
        np.testing.assert_array_equal(g, w, err_msg=name)


# ------------------------------------------------------------ 2. control flow, play mode
@pytest.mark.parametrize("rand", [0, 6])
@pytest.mark.parametrize("flags", [0, 3, 4])
@pytest.mark.parametrize("n", [4, 8])
def test_play_control_flow_is_the_oracles(torch_cuda, n, flags, rand):
    plies = 2 * n * n // 3
    geq = player(torch_cuda, n, pn.geq(n))
    for E in (1, 9, 65):
        kw = dict(initial_rand_steps=rand, seed=11, env_id_base=1000)
        env, twin = make_env(E, n, flags, **kw), make_env(E, n, flags, **kw)
        s = state_of(env)
        ply0 = env.ply_counter
        got = outputs(env.play_ntuple(geq, geq, plies, fallbacks=True, td=True))
        a, r, d, wdl = oracle.rollout(s, flags, 1, plies, seed=11, id_base=1000, ply0=ply0, initial_rand_steps=rand)
        for name, g, w in zip(NAMES, got, (a, r, d)):
            assert g.shape == (plies, E)
            np.testing.assert_array_equal(g, w, err_msg="%s E=%d" % (name, E))
        assert not got[3].any()
        assert_state(env, s, "E=%d" % E)
        np.testing.assert_array_equal(env.counts().cpu().numpy(), wdl)
        for x, y in zip(twin.step_policy("greedy", plies), got):
            np.testing.assert_array_equal(host(x), y)
        assert env.ply_counter == twin.ply_counter == ply0 + plies
        # the rows: a row learns iff its ply moved a live board outside its opening; every other row is zero
        tb, tm, tt, tl = got[4:]
        assert tl.shape == (plies, E) and tb.shape == (plies, E, 2 * env.words) and set(np.unique(tl)) <= {0, 1}
        assert not tb[tl == 0].any() and not tm[tl == 0].any() and not tt[tl == 0].any()
        assert (got[0][tl == 1] >= 0).all() and (E == 1 or tl.sum() > 0)
        env.close()
        twin.close()


# ------------------------------------------------------------ 3. control flow, vs mode
@pytest.mark.parametrize("rand", [0, 6])
@pytest.mark.parametrize("flags", [0, 3, 4])
@pytest.mark.parametrize("who", ["white", "black", "mixed"])
@pytest.mark.parametrize("n", [4, 8])
def test_vs_control_flow_is_the_oracles(torch_cuda, n, who, flags, rand):
    torch = torch_cuda
    E = 65
    prot = {"white": np.ones(E), "black": -np.ones(E), "mixed": np.where(np.arange(E) % 3 == 0, -1, 1)}[who]
    prot = prot.astype(np.int8)
    geq = player(torch, n, pn.geq(n))
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
        np.testing.assert_array_equal(host(d), od, err_msg="dones of call %d" % c)
        np.testing.assert_array_equal(plies.cpu().numpy(), opl, err_msg="plies of call %d" % c)
        assert not fb.any()
        assert_state(env, s, "after call %d" % c)
        fin = live & (od != 0)
        vs += [int((fin & (orw > 0)).sum()), int((fin & (orw == 0)).sum()), int((fin & (orw < 0)).sum())]
    np.testing.assert_array_equal(env.counts().cpu().numpy(), wdl)
    np.testing.assert_array_equal(env.counts_vs().cpu().numpy(), vs)
    assert env.ply_counter == 18
    env.close()


# ------------------------------------------------------------ 4. move choice, vs mode (both first movers)
@pytest.mark.parametrize("explore", [0, 20000])
@pytest.mark.parametrize("first", ["protagonist", "opponent"])
@pytest.mark.parametrize("n", [4, 8])
def test_vs_moves_are_the_references(torch_cuda, n, first, explore):
    torch = torch_cuda
    s = pr.recomputed(sh.batch(n, 74)[0])
    mover = np.where(s.meta & 1, 1, -1).astype(np.int8)
    prot = mover if first == "protagonist" else (-mover).astype(np.int8)
    opp = policies(n)[0]._replace(explore=explore)
    env = make_env(s.E, n, seed=21, env_id_base=77)
    env.ply_counter = 9
    ref = pn.vs_calls(s.copy(), opp, prot, 4, seed=21, id_base=77, call0=9)
    assert sum(int(c[4].sum()) for c in ref) >= 1  # the opponent falls back somewhere
    load(torch, env, s)
    pl = player(torch, n, opp)
    for c, (acts, r, d, plies, fb, after) in enumerate(ref):
        _, gr, gd, gp, gf = env.step_vs(torch.from_numpy(acts).cuda(), pl, protagonist=torch.from_numpy(prot),
                                        observe=False, fallbacks=True)
        for name, g, w in zip(("rewards", "dones", "plies", "fallbacks"), (gr, gd, gp, gf), (r, d, plies, fb)):
            np.testing.assert_array_equal(host(g), w, err_msg="%s of call %d" % (name, c))
        assert_state(env, after, "after call %d" % c)
    assert env.ply_counter == 13
    # the observation of an n-tuple call is observe()'s after it
    twin = make_env(s.E, n)
    load(torch, twin, ref[-1][5])
    load(torch, env, ref[-2][5])
    env.ply_counter = 12
    o = env.step_vs(torch.from_numpy(ref[-1][0]).cuda(), pl, protagonist=torch.from_numpy(prot))[0]
    assert torch.equal(o, twin.get_observation())
    env.close()
    twin.close()


# ------------------------------------------------------------ 5. exploration
_EXPLORE = {}


def explore_reference(explore, E=65, id_base=0):
    key = (explore, E, id_base)
    if key not in _EXPLORE:
        start = sr.subset(pr.recomputed(sh.batch(6, 74)[0]), np.arange(5 + id_base, 5 + id_base + E))
        end = start.copy()
        b, w = policies(6)
        run = pn.play(end, b._replace(explore=explore), w._replace(explore=explore), 6, seed=0x5EED5EED5EED, id_base=id_base,
                      ply0=3)
        _EXPLORE[key] = (start, run, end)
    start, run, end = _EXPLORE[key]
    return start.copy(), run, end


def explore_play(torch, start, explore, id_base=0):
    b, w = policies(6)
    env = make_env(start.E, 6, seed=0x5EED5EED5EED, env_id_base=id_base)
    env.ply_counter = 3
    load(torch, env, start)
    got = outputs(env.play_ntuple(player(torch, 6, b._replace(explore=explore)), player(torch, 6, w._replace(explore=explore)),
                                  6, fallbacks=True, td=True))
    st = state_np(env)
    env.close()
    return got, st


@pytest.mark.parametrize("explore", [0, 16384, 65536])
def test_exploration_is_the_references(torch_cuda, explore):
    start, run, end = explore_reference(explore)
    h = run.held
    assert (h["explored"] == 0) if explore == 0 else (h["explored"] >= 10), dict(h)
    if explore == 16384:  # some plies explore, some search, and some of those fall back
        assert h["learn"] >= 10 and h["fallbacks"] >= 1, dict(h)
    got, st = explore_play(torch_cuda, start, explore)
    for name, g, w in zip(NAMES + TD_NAMES, got, want_of(run, td=True)):
        np.testing.assert_array_equal(g, w, err_msg=name)
    np.testing.assert_array_equal(st[0], end.boards)
    if explore == 65536:  # every move is the purpose-8 draw's, no ply falls back, no row learns
        assert not got[3].any() and not got[7].any()
        s = start.copy()
        ids = rr.ids_from(0, s.E)
        for p in range(6):
            rows = sr.legal_rows(s.legal, 36)
            wants = ((s.meta & 2) == 0) & rows.any(1)
            x = rr.philox4x32_10(0x5EED5EED5EED, ids, 3 + p, 8).astype(np.uint64)
            k = (x[:, 1] * rows.sum(1).astype(np.uint64)) >> np.uint64(32)
            np.testing.assert_array_equal(got[0][p][wants], pn.kth_square(rows, k)[wants])
            live = (s.meta & 2) == 0
            oracle.step(s, 0, np.where(live, got[0][p], 0))


def test_exploration_does_not_depend_on_the_sharding(torch_cuda):
    """Two handles of 32 boards with env_id_base 0 and 32 reproduce one handle of 64."""
    start, run, end = explore_reference(16384, E=64)
    whole, st = explore_play(torch_cuda, start, 16384)
    for name, g, w in zip(NAMES + TD_NAMES, whole, want_of(run, td=True)):
        np.testing.assert_array_equal(g, w, err_msg=name)
    for lo in (0, 32):
        part, pst = explore_play(torch_cuda, sr.subset(start, np.arange(lo, lo + 32)), 16384, id_base=lo)
        for name, g, w in zip(NAMES + TD_NAMES, part, whole):
            np.testing.assert_array_equal(g, w[:, lo:lo + 32], err_msg="%s of the shard at %d" % (name, lo))
        np.testing.assert_array_equal(pst[0], st[0][lo:lo + 32])


# ------------------------------------------------------------ 6. TD rows
_TD = {}
TD_KW = dict(seed=5, id_base=64, ply0=2, initial_rand_steps=4)


def td_reference(n):
    """A run with auto-reset and random openings after it, long enough to end games: (start, Run, end)."""
    if n not in _TD:
        start = pr.recomputed(sh.batch(n, 74)[0])
        end = start.copy()
        run = pn.play(end, *policies(n), PLIES[n] + 2, flags=4, **TD_KW)
        h = run.held
        assert h["ended"] >= 5 and h["resets"] >= 5 and h["passes"] >= 1, dict(h)
        assert h["learn_end"] >= 1 and h["learn_pass"] >= 1 and h["learn_turn"] >= 10, dict(h)
        assert h["fallbacks"] >= 1 and 0 < h["learn"] < run.learn.size, dict(h)
        _TD[n] = (start, run, end)
    start, run, end = _TD[n]
    return start.copy(), run, end


@pytest.mark.parametrize("n", [4, 6, 8])
def test_td_rows_are_the_references(torch_cuda, n):
    torch = torch_cuda
    start, run, end = td_reference(n)
    plies = PLIES[n] + 2
    env = make_env(74, n, 4, seed=5, env_id_base=64, initial_rand_steps=4)
    env.ply_counter = 2
    load(torch, env, start)
    pb, pw = (player(torch, n, p) for p in policies(n))
    before = [pb.net.weights.clone(), pw.net.weights.clone()]
    got = outputs(env.play_ntuple(pb, pw, plies, fallbacks=True, td=True))
    for name, g, w in zip(NAMES + TD_NAMES, got, want_of(run, td=True)):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert_state(env, end)
    np.testing.assert_array_equal(env.counts().cpu().numpy(), run.wdl)
    tb, tm, tt, tl = got[4:]
    assert not tb[tl == 0].any() and not tm[tl == 0].any() and not tt[tl == 0].any()  # learn = 0 rows are all zero
    assert torch.equal(pb.net.weights, before[0]) and torch.equal(pw.net.weights, before[1])  # the weights are frozen
    # without td and without records: the same boards
    env.ply_counter = 2
    load(torch, env, start)
    assert env.play_ntuple(pb, pw, plies, record=False) == (None, None, None)
    assert_state(env, end)
    env.close()


# ------------------------------------------------------------ 7. the masked update and a TD round
@pytest.mark.parametrize("R", [1, 64, 65, 257])
def test_masked_update(torch_cuda, R):
    torch = torch_cuda
    c = nc.case(8, 5, "mixed")
    bd = torch.from_numpy(c.boards[:R].view(np.int64)).cuda()
    mt = torch.from_numpy(c.meta[:R].view(np.int16)).cuda()
    tg = torch.from_numpy(c.targets[:R]).cuda()
    rng = np.random.RandomState(R)
    masks = {"none": np.zeros(R, dtype=np.uint8), "all": np.ones(R, dtype=np.uint8),
             "mixed": (rng.rand(R) < 0.5).astype(np.uint8), "bytes": rng.randint(0, 256, size=R).astype(np.uint8)}
    for name, m in masks.items():
        net = make_net(torch, 8, c.tuples, 3, c.weights)
        d = net.update(bd, mt, tg, 5000, 12, mask=torch.from_numpy(m).cuda())
        want_w, want_d = pn.masked_update(8, c.tuples, 3, c.weights, c.boards[:R], c.meta[:R], c.targets[:R], m, 5000, 12)
        np.testing.assert_array_equal(d.cpu().numpy(), want_d, err_msg="deltas, mask %s" % name)
        np.testing.assert_array_equal(net.weights.cpu().numpy(), want_w, err_msg="weights, mask %s" % name)
        if name == "none":
            assert not want_d.any() and (want_w == c.weights).all()
    # a bool mask; and no mask is oth_ntuple_update
    a, b, plain = (make_net(torch, 8, c.tuples, 3, c.weights) for _ in range(3))
    da = a.update(bd, mt, tg, 5000, 12, mask=torch.from_numpy(masks["mixed"] != 0).cuda())
    assert np.array_equal(da.cpu().numpy(), pn.masked_update(8, c.tuples, 3, c.weights, c.boards[:R], c.meta[:R],
                                                             c.targets[:R], masks["mixed"], 5000, 12)[1])
    lib, st = b._lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    db = torch.full((R,), 7, dtype=torch.int32, device="cuda")
    assert lib.oth_ntuple_update_masked(8, R, ctypes.byref(b.params), ctypes.c_void_p(b.plan.data_ptr()), b.plan_bytes,
                                        ctypes.c_void_p(b.weights.data_ptr()), b.weight_count,
                                        ctypes.c_void_p(bd.data_ptr()), ctypes.c_void_p(mt.data_ptr()),
                                        ctypes.c_void_p(tg.data_ptr()), None, 5000, 12, ctypes.c_void_p(db.data_ptr()),
                                        st) == 0
    dp = plain.update(bd, mt, tg, 5000, 12)
    assert torch.equal(db, dp) and torch.equal(b.weights, plain.weights)
    np.testing.assert_array_equal(plain.weights.cpu().numpy(),
                                  nr.update(8, c.tuples, 3, c.weights, c.boards[:R], c.meta[:R], c.targets[:R], 5000, 12)[0])


def test_td_play_rounds_are_the_references(torch_cuda):
    """Three rounds of td_play (N = 6, E = 64, 8 plies each, a quarter of the plies exploring): the weights
    after every round equal reference play + reference update, bit for bit."""
    torch = torch_cuda
    n, E, plies = 6, 64, 8
    tp, shift, w0 = nc.search_net(n)
    net = make_net(torch, n, tp, shift, w0)
    env = make_env(E, n, 4, seed=13, env_id_base=5, initial_rand_steps=2)
    s = state_of(env)
    rate, rate_shift = net.rate_for(0.5, E * plies)
    assert rate > 0
    w = np.asarray(w0, dtype=np.int32)
    changed = 0
    for k in range(3):
        ply0 = env.ply_counter
        res = net.td_play(env, plies, rate, rate_shift, explore=0.25, depth=1)
        p = pn.pol(tp, shift, w, depth=1, terminal=64, explore=16384)
        run, w_new = pn.td_round(s, p, plies, rate, rate_shift, flags=4, seed=13, id_base=5, ply0=ply0,
                                 initial_rand_steps=2)
        assert run.held["learn"] >= E and run.held["explored"] >= 10, dict(run.held)
        for name, g, want in zip(NAMES[:3] + TD_NAMES, outputs(res), want_of(run, td=True)[:3] + want_of(run, td=True)[4:]):
            np.testing.assert_array_equal(g, want, err_msg="%s of round %d" % (name, k))
        np.testing.assert_array_equal(net.weights.cpu().numpy(), w_new, err_msg="weights after round %d" % k)
        assert_state(env, s, "after round %d" % k)
        assert env.ply_counter == ply0 + plies
        changed += int((w_new != w).sum())
        w = w_new
    assert changed > 100
    env.close()


# ------------------------------------------------------------ 8. cross-check with oth_play_search
@pytest.mark.parametrize("n", [4, 8])
def test_orbit_net_plays_the_piece_counters_moves(torch_cuda, n):
    """A symmetric piece counter as an n-tuple net: oth_play_ntuple gives oth_play_search's bytes."""
    torch = torch_cuda
    from gymothelloenv_amd import SearchConfig
    tp, w, table = nc.orbit_net(n)
    start = pr.recomputed(sh.batch(n, 74)[0])
    pl = player(torch, n, pn.pol(tp, 0, w, depth=2, terminal=64, endgame_empties=3))
    cfg = SearchConfig(depth=2, weights=table, mobility=0, terminal=64, endgame_empties=3)
    res = []
    for call in ("ntuple", "search"):
        env = make_env(start.E, n, 4, seed=3, initial_rand_steps=2)
        load(torch, env, start)
        out = env.play_ntuple(pl, None, PLIES[n] + 2, fallbacks=True) if call == "ntuple" else \
            env.play_search(cfg, None, PLIES[n] + 2, fallbacks=True)
        res.append(([host(t) for t in out], state_np(env)))
        env.close()
    assert (res[0][0][0] >= 0).sum() > 100
    for name, g, w_ in zip(NAMES, res[0][0], res[1][0]):
        assert g.tobytes() == w_.tobytes(), name
    for g, w_ in zip(res[0][1], res[1][1]):
        assert g.tobytes() == w_.tobytes()


# ------------------------------------------------------------ 9. shapes
@pytest.mark.parametrize("E", [1, 7, 8, 9, 63, 64, 65])
def test_shapes_small(torch_cuda, E):
    start, run, end = play_reference(8)
    idx = np.arange(9, 9 + E)
    got, st, _ = dev_play(torch_cuda, sr.subset(start, idx), *policies(8), PLIES[8])
    for name, g, w in zip(NAMES, got, want_of(run)):
        np.testing.assert_array_equal(g, w[:, idx], err_msg=name)
    np.testing.assert_array_equal(st[0], end.boards[idx])
    np.testing.assert_array_equal(st[1], end.meta[idx])


def test_shapes_sparse_and_permuted(torch_cuda):
    """Two boards in three are terminated or finish early (one empty square), so whole groups have no task
    in some rounds while others do; stored masks narrowed to one square; a board's results are those of
    the same board alone and under a permutation."""
    start, _, _ = play_reference(8)
    black, white = policies(8)
    live = np.flatnonzero(((start.meta & 2) == 0) & (pn.empties(start) >= 8))
    short = np.flatnonzero(((start.meta & 2) == 0) & (pn.empties(start) == 1))
    assert len(live) >= 20 and len(short) >= 2
    narrow = start.copy()  # every third live board keeps only the highest square of its stored mask
    rows = sr.legal_rows(narrow.legal, 64)
    for e in live[::3]:
        narrow.legal[e] = sr.mask_words([int(np.flatnonzero(rows[e])[-1])], 8)
    end = narrow.copy()
    run = pn.play(end, black, white, 4)
    want = want_of(run, td=True)
    E = 600
    i = np.arange(E)
    src = np.where(i % 3 == 0, live[(i // 3) % len(live)], np.where(i % 3 == 1, 0, short[i % len(short)]))
    src[300:400] = np.where(i[300:400] % 2 == 0, 0, short[0])  # whole groups that are finished after one round
    assert (start.meta[0] & 2) != 0
    got, st, _ = dev_play(torch_cuda, sr.subset(narrow, src), black, white, 4, td=True)
    for name, g, w in zip(NAMES + TD_NAMES, got, want):
        np.testing.assert_array_equal(g, w[:, src], err_msg=name)
    np.testing.assert_array_equal(st[0], end.boards[src])
    np.testing.assert_array_equal(st[1], end.meta[src])
    one, _, _ = dev_play(torch_cuda, sr.subset(narrow, live[3:4]), black, white, 4, td=True)
    for g, w in zip(one, want):
        np.testing.assert_array_equal(g[:, 0], w[:, live[3]])
    perm = np.random.RandomState(5).permutation(start.E)
    pg, pst, _ = dev_play(torch_cuda, sr.subset(narrow, perm), black, white, 4, td=True)
    for g, w in zip(pg, want):
        np.testing.assert_array_equal(g, w[:, perm])
    np.testing.assert_array_equal(pst[0], end.boards[perm])


def test_two_calls_give_identical_bytes(torch_cuda):
    start, _, _ = play_reference(8)
    b, w = (p._replace(explore=9000) for p in policies(8))
    kw = dict(td=True, flags=4, initial_rand_steps=4, seed=3)
    x = dev_play(torch_cuda, start, b, w, 5, **kw)
    y = dev_play(torch_cuda, start, b, w, 5, **kw)
    for p, q in zip(x[0] + list(x[1]) + [x[2]], y[0] + list(y[1]) + [y[2]]):
        assert p.tobytes() == q.tobytes()


def test_capture_in_a_graph_region(torch_cuda):
    """play_ntuple(n_plies=3, td=True) captured inside graph_region: each replay from the restored state
    draws fresh opening and exploring moves from the region's counter range -- replay r equals an eager
    twin's call at counter base + 3 r -- and the eager counters are untouched."""
    torch = torch_cuda
    E, n, K = 300, 8, 3
    tp, shift, w = nc.search_net(n)
    pl = player(torch, n, pn.pol(tp, shift, w, depth=2, explore=16384))
    kw = dict(initial_rand_steps=6, seed=9)
    env, twin = make_env(E, n, 4, **kw), make_env(E, n, 4, **kw)
    twin.play_ntuple(pl, None, 1, record=False)  # (a warm-up launch before the capture)
    env.reset()
    twin.reset()
    twin.ply_counter = 0
    sd = env.state_dict()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), env.graph_region() as slot:
        out = env.play_ntuple(pl, None, K, fallbacks=True, td=True)
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
        want = twin.play_ntuple(pl, None, K, fallbacks=True, td=True)
        for x, y in zip(outputs(out), outputs(want)):
            assert x.tobytes() == y.tobytes()
        for x, y in zip(env.get_state(), twin.get_state()):
            assert torch.equal(x, y)
        if prev is not None:
            assert not torch.equal(prev, out[0])  # fresh draws per replay
        prev = out[0].clone()
    assert env.ply_counter == 0 and env.graph_offsets(slot)[0] == 2 * K and env.graph_offsets(0) == (0, 0)
    env.close()
    twin.close()


def raw_buffers(torch, E, plies, W):
    a, r = torch.full((plies, E), 77, dtype=torch.int32).cuda(), torch.full((plies, E), 77, dtype=torch.int32).cuda()
    d, f = torch.full((plies, E), 77, dtype=torch.uint8).cuda(), torch.full((plies, E), 77, dtype=torch.uint8).cuda()
    tb = torch.full((plies, E, 2 * W), 77, dtype=torch.int64).cuda()
    tm = torch.full((plies, E), 77, dtype=torch.int16).cuda()
    tt, tl = torch.full((plies, E), 77, dtype=torch.int32).cuda(), torch.full((plies, E), 77, dtype=torch.uint8).cuda()
    p1, f1 = torch.full((E,), 77, dtype=torch.int32).cuda(), torch.full((E,), 77, dtype=torch.int32).cuda()
    return a, r, d, f, tb, tm, tt, tl, p1, f1


def test_a_wrong_plan_changes_nothing_but_the_counter(torch_cuda):
    torch = torch_cuda
    from gymothelloenv_amd import _lib as L
    from gymothelloenv_amd.vec_env import _ptr
    E, n = 37, 8
    tp, shift, w = nc.search_net(n)
    good = player(torch, n, pn.pol(tp, shift, w, depth=2))
    other = [list(t) for t in tp]
    other[3] = [(other[3][0] + 1) % 64]
    for wtp, wshift in ((tp, shift + 1), (other, shift)):  # another shift, another square: the same plan size
        wrong = player(torch, n, pn.pol(wtp, wshift, w, depth=2))
        wrong.net.plan = good.net.plan
        env = make_env(E, n, 4, seed=3)
        env.step_policy("random", 7, record=False)
        env.counts(reset=True)
        lib, h, st = env._lib, env._h, env._stream()
        a, r, d, f, tb, tm, tt, tl, p1, f1 = raw_buffers(torch, E, 2, env.words)
        acts = env.greedy_actions()
        before, ply = state_np(env), env.ply_counter
        rows = L.OthNtupleTd(tb.data_ptr(), tm.data_ptr(), tt.data_ptr(), tl.data_ptr())
        gp, wp = good._policy(env), wrong._policy(env)
        g_, x = ctypes.addressof(gp), ctypes.addressof(wp)
        assert lib.oth_play_ntuple(h, x, g_, 2, _ptr(a), _ptr(r), _ptr(d), _ptr(f), ctypes.addressof(rows), st) == 0
        assert lib.oth_play_ntuple(h, g_, x, 2, _ptr(a), _ptr(r), _ptr(d), _ptr(f), ctypes.addressof(rows), st) == 0
        assert lib.oth_step_vs_ntuple(h, x, _ptr(acts), None, _ptr(r), _ptr(d), _ptr(p1), _ptr(f1), st) == 0
        assert lib.oth_reset_vs_ntuple(h, x, None, None, st) == 0
        torch.cuda.synchronize()
        for t in (a, r, d, f, tb, tm, tt, tl, p1, f1):
            assert (t == 77).all()
        for p, q in zip(before, state_np(env)):
            np.testing.assert_array_equal(p, q)
        assert not env.counts().cpu().numpy().any() and not env.counts_vs().cpu().numpy().any()
        assert env.ply_counter == ply + 2 + 2 + 1 + 1  # the counter has advanced all the same
        env.close()


def test_refusals_touch_nothing(torch_cuda):
    torch = torch_cuda
    from gymothelloenv_amd import _lib as L
    from gymothelloenv_amd.vec_env import _ptr
    E, n = 37, 8
    tp, shift, w = nc.search_net(n)
    good = player(torch, n, pn.pol(tp, shift, w, depth=2))
    env = make_env(E, n, seed=3)
    env.step_policy("random", 7, record=False)
    lib, h, st = env._lib, env._h, env._stream()
    gp = good._policy(env)

    def pol(**fields):
        p = L.OthNtuplePolicy()
        ctypes.memmove(ctypes.byref(p), ctypes.byref(gp), ctypes.sizeof(p))
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    badp = pol()
    badp.params.tuples = 0
    bad = [badp, pol(plan=None), pol(plan=gp.plan + 4), pol(plan_bytes=gp.plan_bytes - 1), pol(weights=None),
           pol(weight_count=gp.weight_count - 1), pol(depth=0), pol(depth=15), pol(terminal_weight=0),
           pol(terminal_weight=32768), pol(endgame_empties=-1), pol(endgame_empties=15), pol(explore=-1),
           pol(explore=65537), pol(max_nodes=0), pol(max_nodes=2 ** 32)]
    a, r, d, f, tb, tm, tt, tl, p1, f1 = raw_buffers(torch, E, 2, env.words)
    acts = torch.zeros(E, dtype=torch.int32).cuda()
    rows = L.OthNtupleTd(tb.data_ptr(), tm.data_ptr(), tt.data_ptr(), tl.data_ptr())
    norows = L.OthNtupleTd(tb.data_ptr(), None, tt.data_ptr(), tl.data_ptr())
    g_, td = ctypes.addressof(gp), ctypes.addressof(rows)
    calls = []
    for b in bad:
        x = ctypes.addressof(b)
        calls += [lambda x=x: lib.oth_play_ntuple(h, x, g_, 2, _ptr(a), _ptr(r), _ptr(d), _ptr(f), td, st),
                  lambda x=x: lib.oth_play_ntuple(h, g_, x, 2, _ptr(a), _ptr(r), _ptr(d), _ptr(f), td, st),
                  lambda x=x: lib.oth_reset_vs_ntuple(h, x, None, None, st),
                  lambda x=x: lib.oth_step_vs_ntuple(h, x, _ptr(acts), None, _ptr(r), _ptr(d), _ptr(p1), _ptr(f1), st)]
    calls += [lambda: lib.oth_play_ntuple(None, g_, g_, 2, _ptr(a), _ptr(r), _ptr(d), _ptr(f), td, st),
              lambda: lib.oth_play_ntuple(h, None, g_, 2, _ptr(a), _ptr(r), _ptr(d), _ptr(f), td, st),
              lambda: lib.oth_play_ntuple(h, g_, None, 2, _ptr(a), _ptr(r), _ptr(d), _ptr(f), td, st),
              lambda: lib.oth_play_ntuple(h, g_, g_, 0, _ptr(a), _ptr(r), _ptr(d), _ptr(f), td, st),
              lambda: lib.oth_play_ntuple(h, g_, g_, 2, _ptr(a), _ptr(r), _ptr(d), _ptr(f), ctypes.addressof(norows), st),
              lambda: lib.oth_reset_vs_ntuple(None, g_, None, None, st),
              lambda: lib.oth_reset_vs_ntuple(h, None, None, None, st),
              lambda: lib.oth_step_vs_ntuple(None, g_, _ptr(acts), None, _ptr(r), _ptr(d), _ptr(p1), _ptr(f1), st),
              lambda: lib.oth_step_vs_ntuple(h, None, _ptr(acts), None, _ptr(r), _ptr(d), _ptr(p1), _ptr(f1), st),
              lambda: lib.oth_step_vs_ntuple(h, g_, None, None, _ptr(r), _ptr(d), _ptr(p1), _ptr(f1), st)]
    before, ply = state_np(env), env.ply_counter
    for k, call in enumerate(calls):
        assert call() == -1, k  # OTH_EINVAL
        assert lib.oth_last_error()
    torch.cuda.synchronize()
    for t in (a, r, d, f, tb, tm, tt, tl, p1, f1):
        assert (t == 77).all()
    for p, q in zip(before, state_np(env)):
        np.testing.assert_array_equal(p, q)
    assert env.ply_counter == ply
    # the Python layer: wrong types and sizes
    import gymothelloenv_amd as g
    with pytest.raises(TypeError):
        env.play_ntuple("greedy")
    with pytest.raises(TypeError):
        env.play_ntuple(good, g.SearchConfig(depth=1))
    with pytest.raises(ValueError):
        env.play_ntuple(good, n_plies=0)
    with pytest.raises(ValueError):
        env.play_ntuple(player(torch, 6, pn.geq(6)))  # another board size's net
    for kwargs in (dict(depth=0), dict(depth=15), dict(endgame_empties=15), dict(explore=-0.1), dict(explore=1.5),
                   dict(terminal=0), dict(max_nodes=0), dict(depth=2.5)):
        with pytest.raises(ValueError):
            g.NTuplePlayer(good.net, **kwargs)
    with pytest.raises(ValueError):
        good.net.update(torch.zeros(4, 2, dtype=torch.int64), torch.zeros(4, dtype=torch.int16),
                        torch.zeros(4, dtype=torch.int32), 1, 0, mask=torch.zeros(3, dtype=torch.uint8))
    assert env.ply_counter == ply
    env.close()


# ------------------------------------------------------------ 10. the Python surface
def test_othello_env_with_an_ntuple_player_opponent(torch_cuda):
    """NTuplePolicy(NTuplePlayer) as OthelloEnv's embedded opponent: its moves are play_ntuple's for the board."""
    torch = torch_cuda
    import gymothelloenv_amd as g
    tp, shift, w = nc.search_net(8)
    pl = player(torch, 8, pn.pol(tp, shift, w, depth=2, endgame_empties=6))
    policy = g.NTuplePolicy(pl)
    assert policy.player is pl and policy.net is pl.net
    env = g.OthelloEnv(black_policy=policy, protagonist=g.WHITE_DISK, board_size=8)
    seen = []
    inner = policy.get_action

    def spy(obs):
        env.env._sync()
        s = state_of(env.env._vec)
        want = pn.moves(s, pn.pol(tp, shift, w, depth=2, endgame_empties=6), pn.pol(tp, shift, w, depth=2, endgame_empties=6))[0]
        a = inner(obs)
        seen.append((a, int(want[0])))
        return a

    policy.get_action = spy
    me = g.RandomPolicy(seed=3)
    with contextlib.redirect_stdout(io.StringIO()):
        obs = env.reset()
        me.reset(env)
        done, plies = False, 0
        while not done and plies < 12:
            obs, _, done, _ = env.step(me.get_action(obs))
            plies += 1
    assert len(seen) >= 8 and all(a == want for a, want in seen)
    env.close()
