"""The n-tuple network on the device -- oth_ntuple_eval, oth_ntuple_update,
oth_search_ntuple and their Python surface (NTupleNet, VecOthelloEnv.search_ntuple,
NTuplePolicy, ntuple_evaluator) -- against the numpy of tests/ntuple_ref.py on the
cases of tests/ntuple_cases.py.  Every comparison is exact equality."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

import mcts_ref as mr
import ntuple_cases as nc
import ntuple_ref as nr
import puct_ref as pf
import search_ref as sh

pytestmark = pytest.mark.gpu

GUARD = 64
NAMES = ("value", "best", "move_values", "status", "nodes")
ALL = dict(best=True, move_values=True, status=True, nodes=True)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def dev(torch, a):
    """A numpy array of the exchange format (or of int32) as the device tensor the package takes."""
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def make_net(torch, n, tp, shift, weights=None):
    import gymothelloenv_amd as g
    net = g.NTupleNet(n, tp, shift, device="cuda:0")
    assert net.weight_count == nr.weight_count(tp) and net.weights.dtype == torch.int32 and not bool(net.weights.any())
    assert net.offsets == nr.offsets(tp)[0]
    if weights is not None:
        net.weights.copy_(torch.from_numpy(np.ascontiguousarray(weights)))
    return net


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def raw_eval(torch, net, bd, mt, R, sums=True):
    """oth_ntuple_eval on the first R rows, into outputs with guard words behind them."""
    values = torch.full((R + GUARD,), 7, dtype=torch.int32, device="cuda")
    sm = torch.full((R + GUARD,), 7, dtype=torch.int64, device="cuda")
    rc = net._lib.oth_ntuple_eval(net.board_size, R, ctypes.byref(net.params), P(net.plan), net.plan_bytes, P(net.weights),
                                  net.weight_count, P(bd), P(mt), P(values), P(sm) if sums else None,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    values, sm = values.cpu().numpy(), sm.cpu().numpy()
    assert (values[R:] == 7).all() and (sm[R:] == 7).all(), "the call wrote behind its output"
    assert sums or (sm == 7).all()
    return values[:R], sm[:R]


@pytest.mark.parametrize("cfg", nc.CONFIGS, ids=nc.CONFIG_IDS)
def test_eval(torch_cuda, cfg):
    torch = torch_cuda
    c = nc.case(*cfg)
    nc.check_rows(c)
    bd, mt = dev(torch, c.boards), dev(torch, c.meta)
    for shift in nc.SHIFTS:
        net = make_net(torch, c.n, c.tuples, shift, c.weights)
        want_v, want_s = nr.evaluate(c.n, c.tuples, shift, c.weights, c.boards, c.meta)
        clamped = np.abs(want_s >> shift) > 32768
        assert clamped.any() if shift == 0 else not clamped.any()
        for R in nc.ROWS:
            v, s = raw_eval(torch, net, bd, mt, R)
            np.testing.assert_array_equal(v, want_v[:R], err_msg="values of %d rows" % R)
            np.testing.assert_array_equal(s, want_s[:R], err_msg="sums of %d rows" % R)
        np.testing.assert_array_equal(raw_eval(torch, net, bd, mt, 65, sums=False)[0], want_v[:65])
        v, s = net.evaluate(bd, mt, sums=True)  # the class
        assert v.dtype == torch.int32 and s.dtype == torch.int64
        np.testing.assert_array_equal(v.cpu().numpy(), want_v)
        np.testing.assert_array_equal(s.cpu().numpy(), want_s)
        only = net.evaluate(bd[:0], mt[:0])
        assert isinstance(only, torch.Tensor) and only.numel() == 0
        assert torch.equal(net.weights.cpu(), torch.from_numpy(c.weights)), "the evaluation wrote the weights"


def test_eval_names_the_plans_geometry(torch_cuda):
    """A call that names other parameters than the plan's writes nothing."""
    torch = torch_cuda
    c = nc.case(8, 5, "mixed")
    net = make_net(torch, 8, c.tuples, 3, c.weights)
    bd, mt = dev(torch, c.boards), dev(torch, c.meta)
    other = [list(t) for t in c.tuples]
    other[3] = [(other[3][0] + 1) % 64]
    for n, tp, shift in ((8, c.tuples, 4), (8, other, 3)):
        wrong = make_net(torch, n, tp, shift, c.weights)
        wrong.plan = net.plan  # (the same size: T is the same)
        v, s = raw_eval(torch, wrong, bd, mt, 257)
        assert (v == 7).all() and (s == 7).all()
        before = wrong.weights.clone()
        d = wrong.update(bd, mt, dev(torch, c.targets), 5000, 12)
        assert torch.equal(wrong.weights, before)
        del d


def raw_update(torch, net, bd, mt, tg, R, rate, rate_shift):
    """oth_ntuple_update on the first R rows with guard words behind the deltas and the weights."""
    count = net.weight_count
    w = torch.full((count + GUARD,), 7, dtype=torch.int32, device="cuda")
    w[:count] = net.weights
    d = torch.full((R + GUARD,), 7, dtype=torch.int32, device="cuda")
    rc = net._lib.oth_ntuple_update(net.board_size, R, ctypes.byref(net.params), P(net.plan), net.plan_bytes, P(w), count,
                                    P(bd), P(mt), P(tg), rate, rate_shift, P(d),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    w, d = w.cpu().numpy(), d.cpu().numpy()
    assert (w[count:] == 7).all() and (d[R:] == 7).all(), "the call wrote behind its output"
    return w[:count], d[:R]


@pytest.mark.parametrize("cfg", nc.CONFIGS, ids=nc.CONFIG_IDS)
def test_update(torch_cuda, cfg):
    torch = torch_cuda
    c = nc.case(*cfg)
    bd, mt, tg = dev(torch, c.boards), dev(torch, c.meta), dev(torch, c.targets)
    for shift, (name, rate, rate_shift) in zip((0, 9, 0, 9, 0), nc.RATES):
        net = make_net(torch, c.n, c.tuples, shift, c.weights)
        for R in (nc.ROWS if name == "plain" else (257,)):
            want_w, want_d = nr.update(c.n, c.tuples, shift, c.weights, c.boards[:R], c.meta[:R], c.targets[:R], rate,
                                       rate_shift)
            w, d = raw_update(torch, net, bd, mt, tg, R, rate, rate_shift)
            np.testing.assert_array_equal(d, want_d, err_msg="%s: deltas of %d rows" % (name, R))
            np.testing.assert_array_equal(w, want_w, err_msg="%s: weights after %d rows" % (name, R))
            if name == "zero":
                assert not d.any() and (w == c.weights).all()
            if name == "largest" and R:
                assert (np.abs(d.astype(np.int64)) == 1 << 30).any(), "no delta reached the clamp"


def test_update_special_cases(torch_cuda):
    torch = torch_cuda
    # maximal contention: every row hits the same three entries eight times
    c = nc.case(4, 1, "ones")
    tp = [[5]]
    w0 = np.array([100, -200, 300, 7], dtype=np.int32)
    bd, mt = dev(torch, c.boards), dev(torch, c.meta)
    net = make_net(torch, 4, tp, 0, w0)
    want_w, want_d = nr.update(4, tp, 0, w0, c.boards, c.meta, c.targets, 3000, 10)
    d = net.update(bd, mt, dev(torch, c.targets), 3000, 10)
    np.testing.assert_array_equal(d.cpu().numpy(), want_d)
    np.testing.assert_array_equal(net.weights.cpu().numpy(), want_w)
    assert (want_w != w0).all()
    # a weight started at 2^31 - 5 wraps
    wrap = np.full(4, 2 ** 31 - 5, dtype=np.int32)
    tg = np.full(257, 40000, dtype=np.int32)
    net = make_net(torch, 4, tp, 24, wrap)
    want_w, want_d = nr.update(4, tp, 24, wrap, c.boards, c.meta, tg, 1, 0)
    assert (want_d > 0).all() and (want_w < 0).all()
    d = net.update(bd, mt, dev(torch, tg), 1, 0)
    np.testing.assert_array_equal(d.cpu().numpy(), want_d)
    np.testing.assert_array_equal(net.weights.cpu().numpy(), want_w)
    # three updates in a row, and an evaluation after each sees the new weights
    c = nc.case(10, 5, "mixed")
    bd, mt, tg = dev(torch, c.boards), dev(torch, c.meta), dev(torch, c.targets)
    net = make_net(torch, 10, c.tuples, 9, c.weights)
    w_ref = c.weights
    for k in range(3):
        w_ref, d_ref = nr.update(10, c.tuples, 9, w_ref, c.boards, c.meta, c.targets, 9000 + k, 10)
        d = net.update(bd, mt, tg, 9000 + k, 10)
        np.testing.assert_array_equal(d.cpu().numpy(), d_ref)
        np.testing.assert_array_equal(net.weights.cpu().numpy(), w_ref)
        np.testing.assert_array_equal(net.evaluate(bd, mt).cpu().numpy(),
                                      nr.evaluate(10, c.tuples, 9, w_ref, c.boards, c.meta)[0])
    assert (w_ref != c.weights).any()


def test_graph_capture(torch_cuda):
    """Eval, update and eval captured into one HIP graph and replayed twice: each replay is the reference's
    evaluation, step and evaluation from where the last one left the weights."""
    torch = torch_cuda
    c = nc.case(8, 5, "mixed")
    bd, mt, tg = dev(torch, c.boards), dev(torch, c.meta), dev(torch, c.targets)
    net = make_net(torch, 8, c.tuples, 9, c.weights)
    warm = make_net(torch, 8, c.tuples, 9, c.weights)  # the kernels are loaded before the capture, on another net
    warm.evaluate(bd, mt)
    warm.update(bd, mt, tg, 9000, 10)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # records only
        before = net.evaluate(bd, mt)
        deltas = net.update(bd, mt, tg, 9000, 10)
        after = net.evaluate(bd, mt)
    torch.cuda.synchronize()
    assert torch.equal(net.weights.cpu(), torch.from_numpy(c.weights)), "the capture ran something"
    w_ref = c.weights
    for _ in range(2):
        for t in (before, deltas, after):
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(before.cpu().numpy(), nr.evaluate(8, c.tuples, 9, w_ref, c.boards, c.meta)[0])
        w_ref, d_ref = nr.update(8, c.tuples, 9, w_ref, c.boards, c.meta, c.targets, 9000, 10)
        np.testing.assert_array_equal(deltas.cpu().numpy(), d_ref)
        np.testing.assert_array_equal(net.weights.cpu().numpy(), w_ref)
        np.testing.assert_array_equal(after.cpu().numpy(), nr.evaluate(8, c.tuples, 9, w_ref, c.boards, c.meta)[0])


def test_learning(torch_cuda):
    """64 delta-rule steps towards a hidden net's values: the reference's mean error never rises and ends below
    half of its start (the numpy prototype ended at 0.07 of it), and the device's weights are the reference's."""
    torch = torch_cuda
    import gymothelloenv_amd as g
    n, rows, steps = 4, 512, 64
    tp = g.snake_tuples(n, 6, 2, seed=11)
    assert len(tp) == 6 and all(len(t) == 2 and len(set(t)) == 2 for t in tp) and tp == g.snake_tuples(n, 6, 2, seed=11)
    for a, b in tp:  # connected: neighbours
        assert max(abs(a // n - b // n), abs(a % n - b % n)) == 1
    boards, meta = nc.rows(n, rows, seed=1)
    hidden = np.random.RandomState(12).randint(-20000, 20001, size=nr.weight_count(tp)).astype(np.int32)
    targets, _ = nr.evaluate(n, tp, 6, hidden, boards, meta)
    net = make_net(torch, n, tp, 6)
    rate, rate_shift = net.rate_for(1, rows)
    assert (rate, rate_shift) == (42799, 24)  # round(2^30 / (49 * 512)) at shift 24: alpha = 1
    bd, mt, tg = dev(torch, boards), dev(torch, meta), dev(torch, targets)
    w = np.zeros_like(hidden)
    errs = []
    for _ in range(steps):
        errs.append(np.abs(targets.astype(np.int64) - nr.evaluate(n, tp, 6, w, boards, meta)[0]).mean())
        w, _ = nr.update(n, tp, 6, w, boards, meta, targets, rate, rate_shift)
        net.update(bd, mt, tg, rate, rate_shift)
    errs.append(np.abs(targets.astype(np.int64) - nr.evaluate(n, tp, 6, w, boards, meta)[0]).mean())
    assert all(b <= a for a, b in zip(errs, errs[1:])), errs
    assert errs[-1] < 0.5 * errs[0], (errs[0], errs[-1])
    np.testing.assert_array_equal(net.weights.cpu().numpy(), w)


def make_env(E, n, **kw):
    from gymothelloenv_amd import VecOthelloEnv
    return VecOthelloEnv(E, board_size=n, device="cuda:0", **kw)


def load(torch, env, s):
    env.set_state(dev(torch, s.boards), dev(torch, s.meta), dev(torch, s.legal))


def outputs(res):
    out = [t.cpu().numpy() for t in res]
    out[4] = out[4].view(np.uint64)
    return out


@pytest.mark.parametrize("n", nc.SIZES)
def test_search(torch_cuda, n):
    torch = torch_cuda
    tp, shift, w = nc.search_net(n)
    net = make_net(torch, n, tp, shift, w)
    env = make_env(nc.SEARCH_E, n)
    for depth in sh.depths(n):
        s, res = nc.search_reference(n, depth)
        assert set(res.status.tolist()) == {sh.DONE, sh.TERMINATED, sh.NO_MOVE}
        load(torch, env, s)
        got = outputs(env.search_ntuple(depth, net, terminal=64, **ALL))
        assert got[0].dtype == np.int32 and got[2].shape == (nc.SEARCH_E, n * n) and got[3].dtype == np.uint8
        for name, g_, want in zip(NAMES, got, res.outputs()):
            np.testing.assert_array_equal(g_, want, err_msg="%s at depth %d" % (name, depth))
        if depth == 2:  # value alone, and the actions
            only = env.search_ntuple(depth, net)
            assert isinstance(only, torch.Tensor)
            np.testing.assert_array_equal(only.cpu().numpy(), res.value)
            np.testing.assert_array_equal(env.search_ntuple_actions(depth=depth, net=net).cpu().numpy(), res.best)
    s, res = nc.search_reference(n, 3, nc.BUDGET)  # a budget that aborts some board, not all
    assert (res.status == sh.ABORTED).any() and (res.status == sh.DONE).any()
    load(torch, env, s)
    got = outputs(env.search_ntuple(3, net, terminal=64, max_nodes=nc.BUDGET, **ALL))
    for name, g_, want in zip(NAMES, got, res.outputs()):
        np.testing.assert_array_equal(g_, want, err_msg="%s under a budget" % name)
    after = env.get_state()
    np.testing.assert_array_equal(after[0].cpu().numpy().view(np.uint64), s.boards)  # the handle is left as it was
    env.close()


@pytest.mark.parametrize("n", (4, 8, 10))
def test_search_is_oth_search_on_a_piece_counter(torch_cuda, n):
    """A net of one 1-tuple per symmetry orbit of squares with w = (0, +x, -x) is a symmetric piece counter:
    oth_search_ntuple gives the bytes oth_search gives on that table, without any reference."""
    torch = torch_cuda
    tp, w, table = nc.orbit_net(n)
    assert len(tp) == {4: 3, 8: 10, 10: 15}[n] and w[-1] == 0
    s, _ = sh.batch(n, nc.SEARCH_E)
    # no value clamps: the reference's sums are the table's weighted disc difference, far inside +-32768
    tw = (s.meta & 1) != 0
    _, sums = nr.evaluate(n, tp, 0, w, s.boards, s.meta)
    nn, W = n * n, (n * n + 63) // 64
    a = np.arange(nn)
    bits = lambda words: ((words[:, a // 64] >> (a % 64).astype(np.uint64)) & np.uint64(1)).astype(np.int64)  # noqa: E731
    diff = (bits(s.boards[:, :W]) - bits(s.boards[:, W:])) @ table.astype(np.int64)
    np.testing.assert_array_equal(sums, np.where(tw, -diff, diff))
    assert np.abs(table.astype(np.int64)).sum() < 32768 and table.any()
    net = make_net(torch, n, tp, 0, w)
    env = make_env(nc.SEARCH_E, n)
    load(torch, env, s)
    for depth in (1, 2, 3):
        for budget in (1 << 22, nc.BUDGET):
            got = env.search_ntuple(depth, net, terminal=64, max_nodes=budget, **ALL)
            want = env.search(depth, table, mobility=0, terminal=64, max_nodes=budget, **ALL)
            for name, x, y in zip(NAMES, got, want):
                assert torch.equal(x, y), "%s at depth %d" % (name, depth)
            assert bool((want[3] == sh.DONE).any())
    env.close()


def test_argument_refusals(torch_cuda):
    """An OTH_EINVAL case launches nothing: outputs pre-filled with a sentinel stay."""
    torch = torch_cuda
    from gymothelloenv_amd import _lib as L
    c = nc.case(8, 5, "mixed")
    net = make_net(torch, 8, c.tuples, 3, c.weights)
    bd, mt = dev(torch, c.boards), dev(torch, c.meta)
    out = torch.full((257,), 77, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib, p = net._lib, ctypes.byref(net.params)
    assert lib.oth_ntuple_eval(8, 257, p, P(net.plan), net.plan_bytes - 1, P(net.weights), net.weight_count, P(bd), P(mt),
                               P(out), None, stream) == -1
    assert lib.oth_ntuple_eval(8, 257, p, P(net.plan), net.plan_bytes, P(net.weights), net.weight_count - 1, P(bd), P(mt),
                               P(out), None, stream) == -1
    assert lib.oth_ntuple_update(8, 257, p, P(net.plan), net.plan_bytes, P(net.weights), net.weight_count, P(bd), P(mt),
                                 P(out), (1 << 24) + 1, 0, P(out), stream) == -1
    env = make_env(257, 8)
    assert lib.oth_search_ntuple(env._h, 15, p, P(net.plan), net.plan_bytes, P(net.weights), net.weight_count, 64, 1 << 20,
                                 P(out), None, None, None, None, stream) == -1
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and torch.equal(net.weights.cpu(), torch.from_numpy(c.weights))
    with pytest.raises(L.OthelloLibError, match="depth"):
        env.search_ntuple(15, net)
    with pytest.raises(ValueError, match="boards"):
        env.search_ntuple(2, make_net(torch, 6, nc.tuples(6, 5, "mixed"), 3))
    env.close()


def test_ntuple_policy_moves_are_the_searchs(torch_cuda):
    torch = torch_cuda
    import gymothelloenv_amd as g
    tp, shift, w = nc.search_net(8)
    net = make_net(torch, 8, tp, shift, w)
    policy = g.NTuplePolicy(net, depth=2)
    env = g.OthelloEnv(black_policy=g.RandomPolicy(seed=3), protagonist=g.WHITE_DISK, board_size=8)
    twin = make_env(1, 8)
    with contextlib.redirect_stdout(io.StringIO()):
        obs = env.reset()
        policy.reset(env)
        done, plies = False, 0
        while not done and plies < 10:
            env.env._sync()
            twin.set_state(*env.env._vec.get_state())
            want = int(twin.search_ntuple_actions(depth=2, net=net).cpu()[0])
            a = policy.get_action(obs)
            assert a == want and a in env.possible_moves
            obs, _, done, _ = env.step(a)
            plies += 1
    assert plies >= 6
    twin.close()


def test_ntuple_evaluator_in_puct_search(torch_cuda):
    """puct_search(ntuple_evaluator(net), 8) on 16 boards: tests/puct_ref.py fed the same values (the
    reference's leaves valued by ntuple_ref, the priors puct_quantize makes of zero logits on them)."""
    torch = torch_cuda
    import gymothelloenv_amd as g
    n, E, S = 8, 16, 8
    tp, shift, w = nc.search_net(n)
    net = make_net(torch, n, tp, shift, w)
    s = mr.positions(n, E)
    env = make_env(E, n)
    load(torch, env, s)
    T = S * (n * n - 4) // 4 + n * n
    got = env.puct_search(g.ntuple_evaluator(net), S, value_sums=True, best=True, tree_nodes=True, status=True)
    ref = pf.Search(s, 320, T)
    nonzero = 0
    for i in range(S):
        _, boards, meta, legal = ref.leaves()
        values, _ = nr.evaluate(n, tp, shift, w, boards, meta)
        nonzero += int((values != 0).sum())
        priors, vq = g.puct_quantize(torch.zeros(E, n * n, device="cuda"), dev(torch, legal),
                                     torch.from_numpy(values).cuda().float() / 32768.0)
        np.testing.assert_array_equal(vq.cpu().numpy(), values)  # the float round trip is exact
        ref.advance(priors.cpu().numpy(), values, more=i < S - 1)
    assert nonzero > E
    for name, x, want in zip(pf.NAMES, got, ref.result()):
        np.testing.assert_array_equal(x.cpu().numpy(), want, err_msg=name)
    env.close()
