"""oth_puct_noise and VecOthelloEnv.puct_noise on the device against the Python
integers of tests/noise_ref.py: the host test's table of cases bit for bit, a captured
call, and whole self-play moves through puct_play(..., noise=RootNoise(...)) against
the reference's loops.  Every comparison with the reference is exact equality."""
import numpy as np
import pytest

import mcts_ref as mr
import net_cases as nc
import net_ref as nr
import noise_cases as nz
import noise_ref as nf
from test_gpu_puct import load, make_env, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(torch, a, view=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if view is None else a.view(view)).to(DEV)


def case_env(torch, c):
    """An env that holds the case's boards and possible_moves."""
    from gymothelloenv_amd import PuctLeaves
    env = make_env(nz.E, c.n, seed=1, env_id_base=c.id_base)
    env.set_state(dev(torch, c.handle_boards, np.int64), torch.zeros(nz.E, dtype=torch.int16, device=DEV),
                  dev(torch, c.handle_legal, np.int64))
    leaves = None
    if c.kind is not None:
        leaves = PuctLeaves(dev(torch, c.kind), dev(torch, c.boards, np.int64), None, None, None)
    return env, leaves, dev(torch, c.table.astype(np.uint32), np.int32)


def run(torch, env, leaves, table, c, epsilon, inplace):
    """puct_noise on case c: the output (E K, nn), with guard rows behind it that no call may touch."""
    nn = c.n * c.n
    rows = nz.E * c.K
    whole = torch.full((rows + 2, nn), 7, dtype=torch.int32, device=DEV)
    out = whole[:rows]
    src = dev(torch, c.priors)
    if inplace:
        out.copy_(src)
        src = out
    got = env.puct_noise(src, epsilon, table, leaves=leaves, rows_per_board=c.K, out=out, seed=c.seed, id_key=c.id_key,
                         counter=c.counter)
    assert got is out
    assert bool((whole[rows:] == 7).all()), "the call wrote behind its output"
    if not inplace:
        assert bool((src == dev(torch, c.priors)).all()), "the call wrote its input"
    return out.cpu().numpy()


@pytest.mark.parametrize("key", nz.TABLE_KEYS, ids=nz.TABLE_IDS)
def test_exact_against_the_reference(torch_cuda, key):
    torch = torch_cuda
    n, K, mode, inplace = key
    c = nz.make(n, K, mode)
    env, leaves, table = case_env(torch, c)
    before = [t.clone() for t in env.get_state()]
    for epsilon in nz.EPSILONS:
        want, _ = nz.expected(c, epsilon)
        np.testing.assert_array_equal(run(torch, env, leaves, table, c, epsilon, inplace), want,
                                      err_msg="epsilon %d" % epsilon)
    for x, y in zip(env.get_state(), before):
        assert torch.equal(x, y), "the call wrote the handle"
    env.close()


@pytest.mark.parametrize("i", range(len(nz.SPECIAL)), ids=nz.SPECIAL_IDS)
def test_special_cases(torch_cuda, i):
    torch = torch_cuda
    name, kw = nz.SPECIAL[i]
    c = nz.make(**kw)
    env, leaves, table = case_env(torch, c)
    for epsilon in (64, 256):
        want, _ = nz.expected(c, epsilon)
        for inplace in (False, True):
            np.testing.assert_array_equal(run(torch, env, leaves, table, c, epsilon, inplace), want, err_msg=name)
    env.close()


def test_defaults_and_the_counter(torch_cuda):
    """seed=None is the env's seed XOR PLAYOUT_SEED_XOR, counter=None the env's own, one on a call; out=None a
    new tensor; a sharded run (env_id_base) equals the unsharded one."""
    torch = torch_cuda
    c = nz.make(8, 1, "root")
    env, _, table = case_env(torch, c)
    env.puct_noise_counter = 2 ** 40
    src = dev(torch, c.priors)
    key = (1 ^ nf.PLAYOUT_SEED_XOR) & (2 ** 64 - 1)
    for step in range(2):
        got = env.puct_noise(src, 64, table)
        assert got is not src and bool((src == dev(torch, c.priors)).all())
        want, _ = nf.noise(c.n, c.handle_boards, c.handle_legal, c.priors, 64, c.table, key, 0, 0, 2 ** 40 + step)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert env.puct_noise_counter == 2 ** 40 + 2
    env.puct_noise(src, 64, table, counter=9)
    assert env.puct_noise_counter == 2 ** 40 + 2
    whole = env.puct_noise(src, 64, table, counter=9).cpu().numpy()
    env.close()
    lo = 41
    shard = make_env(nz.E - lo, c.n, seed=1, env_id_base=lo)
    shard.set_state(dev(torch, c.handle_boards[lo:], np.int64), torch.zeros(nz.E - lo, dtype=torch.int16, device=DEV),
                    dev(torch, c.handle_legal[lo:], np.int64))
    part = shard.puct_noise(dev(torch, c.priors[lo:]), 64, table, counter=9).cpu().numpy()
    np.testing.assert_array_equal(part, whole[lo:])
    for bad in (dict(epsilon=257), dict(epsilon=-1), dict(rows_per_board=0), dict(rows_per_board=2)):
        kw = dict(epsilon=64, rows_per_board=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            shard.puct_noise(dev(torch, c.priors[lo:]), kw["epsilon"], table, rows_per_board=kw["rows_per_board"])
    shard.close()


def test_rows_beyond_31_bits_are_refused(torch_cuda):
    """E K = (2^25 + 1) 64 does not fit 31 bits: OTH_EINVAL with nothing launched (the arrays are never read)."""
    import ctypes
    torch = torch_cuda
    env = make_env(2 ** 25 + 1, 4)
    small = torch.full((64,), 7, dtype=torch.int32, device=DEV)
    p = ctypes.c_void_p(small.data_ptr())
    rc = env._lib.oth_puct_noise(env._h, 64, None, None, p, p, 64, p, 1, 0, 0, env._stream())
    assert rc == -1 and b"31 bits" in env._lib.oth_last_error()
    assert env._lib.oth_puct_noise(env._h, 63, None, None, None, p, 64, p, 1, 0, 0, env._stream()) == -1
    torch.cuda.synchronize()
    assert bool((small == 7).all())
    env.close()


def test_captured_call_replays_its_draw(torch_cuda):
    """One leaf-mode call captured in a graph and replayed twice: the counter is baked in, so both replays give
    the eager call's output from the same input."""
    torch = torch_cuda
    c = nz.make(10, 3, "leaf")
    env, leaves, table = case_env(torch, c)
    want, _ = nz.expected(c, 64)
    src = dev(torch, c.priors)
    out = torch.zeros_like(src)
    env.puct_noise(src, 64, table, leaves=leaves, rows_per_board=c.K, out=out, seed=c.seed, counter=c.counter)  # warm
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.puct_noise(src, 64, table, leaves=leaves, rows_per_board=c.K, out=out, seed=c.seed, counter=c.counter)
    for _ in range(2):
        out.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), want)
    env.close()


# ------------------------------------------------------------------ whole self-play moves
S, MOVES, C256 = 16, 8, 320
SAMPLES = [m < 4 for m in range(MOVES)]


def net_of(n):
    """(the reference network, its weights) for a board size: tests/net_cases.py's."""
    if n == 6:
        c = nc.case(nc.TABLE.index((6, 15, 1, 128)))
        return c.net, (c.weights, c.biases, c.shifts, c.policy_shift, c.value_shift)
    weights, biases = nc.draw_weights(n, 2, 64, "mixed", np.random.default_rng(77))
    args = (weights, biases, [5, 9], 8, 2)
    return nr.Net(n, *args), args


def evaluators(torch, n, which):
    """(the device's evaluator, the reference's, puct_play's layout keywords)."""
    import gymothelloenv_amd as g
    if which == "net":
        net, args = net_of(n)
        return g.DeviceNet(n, *args, device=DEV), nf.net_eval(net), dict(layout=None)

    def uniform_on_device(boards, meta, legal):
        # puct_quantize's float32 softmax is the device's: the reference takes its integers from the same code
        rows = boards.shape[0]
        leaves = g.PuctLeaves(torch.ones(rows, dtype=torch.uint8, device=DEV), dev(torch, boards, np.int64),
                              dev(torch, meta, np.int16), dev(torch, legal, np.int64),
                              torch.empty(rows, 1, n, n, device=DEV))
        logits, values = g.uniform_evaluator(leaves)
        priors, values = g.puct_quantize(logits, leaves.legal, values)
        return priors.cpu().numpy(), values.cpu().numpy()

    return g.uniform_evaluator, uniform_on_device, {}


def tree_nodes(n):
    nn = n * n
    return 2 * (S * (nn - 4) // 4 + nn)


def reference_game(s, evaluate, K, epsilon, table):
    if K == 1:
        return nf.PlayGame(s, evaluate, S, SAMPLES, C256, tree_nodes(s.n), epsilon, table, seed=5)
    return nf.BatchGame(s, evaluate, S, SAMPLES, C256, tree_nodes(s.n), K, epsilon, table, seed=5)


def play(torch, s, evaluate, K, noise, kw):
    """MOVES calls of puct_play on the boards of s: a list of PuctPlay as numpy."""
    env = make_env(s.E, s.n, seed=5)
    load(torch, env, s)
    extra = dict(kw)
    if K != 1:
        extra["leaves_per_board"] = K
    if noise is not None:
        extra["noise"] = noise
    moves = []
    for m in range(MOVES):
        out = env.puct_play(evaluate, S, sample=SAMPLES[m], c=C256 / 256.0, max_tree_nodes=tree_nodes(s.n), **extra)
        moves.append(dict(actions=out.actions.cpu().numpy(), visits=out.visits.cpu().numpy(),
                          kept=out.kept.cpu().numpy(), rewards=out.rewards.cpu().numpy(),
                          dones=out.dones.cpu().numpy().astype(np.uint8)))
    counters = (env.puct_noise_counter, env.puct_pick_counter)
    env.close()
    return moves, counters


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("which", ("uniform", "net"))
@pytest.mark.parametrize("n", (6, 10))
def test_self_play_against_the_reference(torch_cuda, n, which, K):
    torch = torch_cuda
    from gymothelloenv_amd import RootNoise
    noise = RootNoise(epsilon=0.25, alpha=0.3)
    s = mr.positions(n, 70)
    on_device, by_reference, kw = evaluators(torch, n, which)
    want = reference_game(s, by_reference, K, noise.epsilon, noise.table.numpy())
    got, (noise_calls, pick_calls) = play(torch, s, on_device, K, noise, kw)
    for m, (g, w) in enumerate(zip(got, want.moves)):
        for name in ("visits", "actions", "rewards", "dones", "kept"):
            np.testing.assert_array_equal(g[name], w[name], err_msg="move %d %s" % (m, name))
    assert pick_calls == sum(SAMPLES)
    assert MOVES < noise_calls <= 2 * MOVES
    assert sum(int(w["kept"].sum()) for w in want.moves) > MOVES and want.moves[-1]["dones"].sum() < 70


@pytest.mark.parametrize("K", (1, 3))
def test_epsilon_zero_is_no_noise_and_noise_changes_the_search(torch_cuda, K):
    torch = torch_cuda
    from gymothelloenv_amd import RootNoise
    n = 6
    s = mr.positions(n, 70)
    on_device, _, kw = evaluators(torch, n, "net")
    plain, (calls, _) = play(torch, s, on_device, K, None, kw)
    assert calls == 0, "without the keyword nothing draws"
    zero, _ = play(torch, s, on_device, K, RootNoise(epsilon=0.0, alpha=0.3), kw)
    for m, (g, w) in enumerate(zip(zero, plain)):
        for name in ("visits", "actions", "rewards", "dones", "kept"):
            np.testing.assert_array_equal(g[name], w[name], err_msg="move %d %s" % (m, name))
    noisy, _ = play(torch, s, on_device, K, RootNoise(epsilon=0.25, alpha=0.3), kw)
    assert (noisy[0]["visits"] != plain[0]["visits"]).any(1).sum() >= 1, "no board's visits differ under noise"
    again, _ = play(torch, s, on_device, K, RootNoise(epsilon=0.25, alpha=0.3), kw)
    for g, w in zip(again, noisy):
        np.testing.assert_array_equal(g["visits"], w["visits"])
