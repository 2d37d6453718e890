"""oth_cnet_eval and DeviceConvNet on the device against the numpy and Python integers
of tests/cnet_ref.py: the tap and operand layout first, then every case of
tests/cnet_cases.py, rows in chunks, another blob's shifts, the network as the
evaluator of a search (against puct_ref / puct_batch_ref driven by cnet_ref), inside a
captured graph and on the replay store's rows.  Every comparison is exact equality."""
import ctypes

import numpy as np
import pytest

import cnet_cases as cc
import cnet_ref as cr
import mcts_ref as mr
import net_ref as nr
import puct_batch_ref as pb
import puct_ref as pf

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def make_env(E, n, seed=0, **kw):
    from gymothelloenv_amd import VecOthelloEnv
    return VecOthelloEnv(E, board_size=n, seed=seed, device=DEV, **kw)


def device_net(c):
    from gymothelloenv_amd import DeviceConvNet
    return DeviceConvNet(c.n, *cc.net_args(c), device=DEV)


def dev(torch, a, view):
    return torch.from_numpy(np.array(a).view(view)).to(DEV)  # (a copy: the cases are read-only)


def rows_np(rows):
    """boards, meta, legal of a PuctLeaves or a ReplayBatch as the reference takes them."""
    return (rows.boards.cpu().numpy().view(np.uint64), rows.meta.cpu().numpy().view(np.uint16),
            rows.legal.cpu().numpy().view(np.uint64))


def evaluate(torch, net, boards, meta, legal, logits=True):
    out = net.evaluate(dev(torch, boards, np.int64), dev(torch, meta, np.int16), dev(torch, legal, np.int64),
                       logits=logits)
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("n", (4, 5, 16))
def test_tap_and_operand_layout(torch_cuda, n):
    """C = 64, B = 1, weights that depend on (o, i, ky, kx) asymmetrically, one-hot rows over every square and
    plane: a transposed tap, a swapped A / B map, a wrong k order or a halo that leaks changes the logits."""
    torch = torch_cuda
    c = cc.layout_case(n)  # (tests/test_cnet_census_cpu.py holds what the case is there for)
    assert len({c.logits[f].tobytes() for f in range(c.R)}) == c.R  # every row's logits are its own
    net = device_net(c)
    priors, values, logits = evaluate(torch, net, c.boards, c.meta, c.legal)
    np.testing.assert_array_equal(logits, c.logits)
    np.testing.assert_array_equal(values, c.values)
    np.testing.assert_array_equal(priors, c.priors)


@pytest.mark.parametrize("i", range(len(cc.TABLE)), ids=cc.IDS)
def test_exact_against_the_reference(torch_cuda, i):
    torch = torch_cuda
    c = cc.case(i)
    net = device_net(c)
    priors, values, logits = evaluate(torch, net, c.boards, c.meta, c.legal)
    np.testing.assert_array_equal(logits, c.logits)
    np.testing.assert_array_equal(values, c.values)
    np.testing.assert_array_equal(priors, c.priors)
    p2, v2 = evaluate(torch, net, c.boards, c.meta, c.legal, logits=False)
    assert (p2 == priors).all() and (v2 == values).all()


@pytest.mark.parametrize("i", (cc.TABLE.index((8, 67, 3, 64)), cc.TABLE.index((5, 17, 1, 64))), ids=lambda i: cc.IDS[i])
def test_rows_are_independent(torch_cuda, i):
    """Whole and in chunks of 1, 16 and 17 rows: the same rows (8 x 8: a row a workgroup; 5 x 5: two)."""
    torch = torch_cuda
    c = cc.case(i)
    net = device_net(c)
    for chunk in (1, 16, 17):
        for lo in range(0, c.R, chunk):
            hi = min(c.R, lo + chunk)
            priors, values, logits = evaluate(torch, net, c.boards[lo:hi], c.meta[lo:hi], c.legal[lo:hi])
            np.testing.assert_array_equal(logits, c.logits[lo:hi])
            np.testing.assert_array_equal(values, c.values[lo:hi])
            np.testing.assert_array_equal(priors, c.priors[lo:hi])


def test_the_c_call_on_a_part_and_other_shifts(torch_cuda):
    """The C call on the first 33 rows of arrays that hold 67: rows 33 .. 66 keep their fill.  A blob packed for
    other shifts, or another blob's parameters, writes nothing."""
    torch = torch_cuda
    from gymothelloenv_amd import DeviceConvNet
    from gymothelloenv_amd import _lib as L
    c = cc.case(cc.TABLE.index((8, 67, 3, 64)))
    net = device_net(c)
    lib = L.load()
    b, m, lg = dev(torch, c.boards, np.int64), dev(torch, c.meta, np.int16), dev(torch, c.legal, np.int64)
    priors = torch.full((c.R, c.nn), 7, dtype=torch.int32, device=DEV)
    values = torch.full((c.R,), 7, dtype=torch.int32, device=DEV)
    logits = torch.full((c.R, c.nn + 1), 7, dtype=torch.int32, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.oth_cnet_eval(c.n, 33, ctypes.byref(net.params), P(net.blob), net.blob.numel(), P(b), P(m), P(lg),
                              P(priors), P(values), P(logits), stream), "oth_cnet_eval")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(priors[:33].cpu().numpy(), c.priors[:33])
    np.testing.assert_array_equal(values[:33].cpu().numpy(), c.values[:33])
    np.testing.assert_array_equal(logits[:33].cpu().numpy(), c.logits[:33])
    assert bool((priors[33:] == 7).all()) and bool((values[33:] == 7).all()) and bool((logits[33:] == 7).all())
    # a blob packed for other shifts, evaluated with this net's parameters; and this blob with other parameters
    args = list(cc.net_args(c))
    args[3] = [c.shifts[0] + 1] + list(c.shifts[1:])
    other = DeviceConvNet(c.n, *args, device=DEV)
    assert other.blob.numel() == net.blob.numel()
    for params, blob in ((net.params, other.blob), (other.params, net.blob)):
        priors.fill_(7)
        values.fill_(7)
        logits.fill_(7)
        L.check(lib.oth_cnet_eval(c.n, c.R, ctypes.byref(params), P(blob), blob.numel(), P(b), P(m), P(lg),
                                  P(priors), P(values), P(logits), stream), "oth_cnet_eval")
        torch.cuda.synchronize()
        assert bool((priors == 7).all()) and bool((values == 7).all()) and bool((logits == 7).all())
    for field, v in (("policy_shift", c.policy_shift + 1), ("value_shift", c.value_shift + 1),
                     ("shift_stem", c.shift_stem + 1), ("shift_head", c.shift_head + 1)):
        p2 = L.OthCnetParams.from_buffer_copy(net.params)
        setattr(p2, field, v)
        L.check(lib.oth_cnet_eval(c.n, c.R, ctypes.byref(p2), P(net.blob), net.blob.numel(), P(b), P(m), P(lg),
                                  P(priors), P(values), None, stream), "oth_cnet_eval")
        torch.cuda.synchronize()
        assert bool((priors == 7).all()) and bool((values == 7).all()), field


SEARCH_CASE = cc.TABLE.index((6, 15, 2, 128))


@pytest.mark.parametrize("K", (1, 4))
def test_a_whole_search(torch_cuda, K):
    """puct_search on 5 boards of 6 x 6, 24 simulations, with a DeviceConvNet: the visit counts of puct_ref (K = 1)
    and puct_batch_ref (K = 4) driven by cnet_ref."""
    torch = torch_cuda
    n, E, S, C, T = 6, 5, 24, 320, 1024
    c = cc.case(SEARCH_CASE)
    net = device_net(c)
    s = mr.positions(n, E)
    env = make_env(E, n, seed=5)
    env.set_state(torch.from_numpy(s.boards.view(np.int64)).to(DEV), torch.from_numpy(s.meta.view(np.int16)).to(DEV),
                  torch.from_numpy(s.legal.view(np.int64)).to(DEV))
    got = env.puct_search(net, S, leaves_per_board=K, c=C / 256.0, max_tree_nodes=T, layout=None).cpu().numpy()
    ref = pf.Search(s.copy(), C, T) if K == 1 else pb.Search(s.copy(), C, T, K)
    if K == 1:
        for i in range(S):
            _, boards, meta, legal = ref.leaves()
            priors, values, _ = c.net.evaluate(boards, meta, legal)
            ref.advance(priors, values, more=i < S - 1)
    else:
        launches = 0
        while ref.leaves()[0].any():
            _, boards, meta, legal = ref.leaves()
            priors, values, _ = c.net.evaluate(boards, meta, legal)
            ref.advance(priors, values, S)
            launches += 1
        assert launches < S
    want = ref.result()[0]
    np.testing.assert_array_equal(got, want)
    assert int(want.sum(1).max()) == S - 1 and len(set(map(bytes, want))) > 1
    env.close()


def test_an_evaluation_in_a_captured_graph(torch_cuda):
    """One evaluation captured on a single stream and replayed equals the eager one, also on rows written after the
    capture."""
    torch = torch_cuda
    c = cc.case(cc.TABLE.index((10, 19, 2, 64)))
    net = device_net(c)
    b, m, lg = dev(torch, c.boards, np.int64), dev(torch, c.meta, np.int16), dev(torch, c.legal, np.int64)
    eager = [t.clone() for t in net.evaluate(b, m, lg)]
    sb, sm, sl = torch.zeros_like(b), torch.zeros_like(m), torch.zeros_like(lg)
    net.evaluate(sb, sm, sl)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        priors, values = net.evaluate(sb, sm, sl)
    sb.copy_(b)
    sm.copy_(m)
    sl.copy_(lg)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(priors, eager[0]) and torch.equal(values, eager[1])
    np.testing.assert_array_equal(priors.cpu().numpy(), c.priors)
    np.testing.assert_array_equal(values.cpu().numpy(), c.values)


def test_replay_rows(torch_cuda):
    """DeviceConvNet on a replay_sample (labelled rows under random symmetries) of self-play games that the net
    itself played to their ends on 4 x 4 is the reference on the batch's rows."""
    torch = torch_cuda
    n, E, H = 4, 8, 16
    c = cc.case(cc.TABLE.index((4, 1, 1, 64)))
    net = device_net(c)
    env = make_env(E, n, seed=3, auto_reset=True)
    env.reset()
    env.replay_begin(H, max_batch=64)
    for _ in range(14):  # a 4 x 4 game has at most 12 moves: every board ends one
        env.puct_play(net, 4, record=True, layout=None)
    batch = env.replay_sample(37, augment=True, seed=11, counter=0, layout=None)
    assert int((batch.state != 0).sum()) == 37 and len(set(batch.sym.cpu().tolist())) > 2
    priors, values = net(batch)
    want = c.net.evaluate(*rows_np(batch))
    np.testing.assert_array_equal(priors.cpu().numpy(), want[0])
    np.testing.assert_array_equal(values.cpu().numpy(), want[1])
    env.close()
