"""The device's random draws against tests/rng_ref.py (an independent numpy
statement of Philox4x32-10 and the opening-length hash) and the CPU oracle,
over 64-bit seeds and counters and env ids up to 2^32 - 1: the sampler's
uniforms, the opening-length draw of every kernel family that resets a board,
oracle replays across the carries of the ply counter, sensitivity to the upper
key bits, and the chi-square statistics of test_rng_spec_cpu.py on what the
kernels return.

Fixture position "one empty square": black holds every square but 0 and 1,
white holds square 1, black is to move.  possible_moves is {0} and playing it
fills the board, so every policy ends every game in one ply and, with
auto-reset, meta >> 8 is that ply's auto-reset draw."""
import numpy as np
import pytest

import rng_ref as R
from oracle import oracle
from test_gpu_parity import get_state_np, make_env, t64
from test_rng_spec_cpu import (GOLDEN, K, OPENING_BOUNDS, PICK_BOUNDS, SD_AUTO, SENSITIVITY_PAIRS, STAT_E, STAT_IDS,
                               check_bounds, opening_families, pick_families, start_moves)

pytestmark = pytest.mark.gpu

SEEDS = (5, GOLDEN, 1 << 32)
PLIES64 = (0, 2 ** 32 - 1, (5 << 40) + 3)
E_RAGGED = 5001


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def one_empty_square(n, E):
    s = oracle.State(n, E)
    nn = n * n
    for w in range(s.W):
        full = (1 << min(64, nn - 64 * w)) - 1
        s.boards[:, w] = np.uint64(full & ~3 if w == 0 else full)
    s.boards[:, s.W] = np.uint64(2)
    s.meta[:] = 0  # black to move, live
    s.legal[:] = oracle.recompute_legal(s)
    assert (s.legal[:, 0] == 1).all() and not s.legal[:, 1:].any()
    return s


def load(torch, env, s):
    env.set_state(t64(torch, s.boards), torch.from_numpy(s.meta.view(np.int16)).cuda(), t64(torch, s.legal))


def assert_start_with(env, want_len, what, rows=slice(None)):
    """The env's boards `rows` are the start position (black to move, live) with
    want_len random-opening plies to play."""
    b, m, lg = get_state_np(env)
    ref = oracle.reset(env.board_size, 1)
    assert (b[rows] == ref.boards[0]).all(), what + ": not the start position"
    assert (lg[rows] == ref.legal[0]).all(), what + ": possible_moves are not the start position's"
    assert ((m[rows] & 0xff) == 0).all(), what + ": turn / terminated / winner bits set"
    np.testing.assert_array_equal(m[rows] >> 8, want_len, what)


def all_legal(n, E):
    lg = np.zeros((E, oracle.nwords(n)), dtype=np.uint64)
    for w in range(lg.shape[1]):
        lg[:, w] = np.uint64((1 << min(64, n * n - 64 * w)) - 1)
    return lg


# ------------------------------------------------------ (a) sampler known answers
@pytest.mark.parametrize("n,shift", [(4, 28), (8, 26), (16, 24)])
def test_masked_sample_draws_the_reference_word(torch_cuda, n, shift):
    """Equal logits over N*N legal squares: the masses are 1, the total a power of
    two and u = (x >> 8) * 2^-24, so the sampled square is exactly x >> shift
    for x = Philox word 0 of (seed, id, counter, purpose 3)."""
    torch = torch_cuda
    from gymothelloenv_amd import masked_sample
    E = 4096
    logits = torch.full((E, n * n), 1.25, dtype=torch.float32, device="cuda:0")
    legal = t64(torch, all_legal(n, E))
    for seed in SEEDS:
        for counter in (1, 2 ** 32 - 1, 2 ** 32, (5 << 40) + 3):
            for id_base in (0, 2 ** 32 - 4096):
                acts, _, _ = masked_sample(logits, legal, n, seed=seed, id_base=id_base, counter=counter)
                want = R.sample_word(seed, R.ids_from(id_base, E), counter) >> shift
                np.testing.assert_array_equal(acts.cpu().numpy(), want,
                                              "seed %#x counter %#x id_base %#x" % (seed, counter, id_base))


@pytest.mark.parametrize("n,E,shift", [(8, 2049, 26), (8, 40000, 26), (16, 1000, 24)])
def test_env_samplers_draw_the_reference_word(torch_cuda, n, E, shift):
    """The same through sample_actions and through every lane layout of
    sample_step (quads, pairs, one lane per board), with the sample counter at
    and above 2^32 and env ids up to 2^32 - 1."""
    torch = torch_cuda
    logits = torch.full((E, n * n), -0.5, dtype=torch.float32, device="cuda:0")
    for seed, id_base, counter in ((GOLDEN, 2 ** 32 - E, 2 ** 32), (1 << 32, 0, (5 << 40) + 3)):
        env = make_env(torch, E, n, auto=True, seed=seed, id_base=id_base)
        b, m, _ = get_state_np(env)
        s = oracle.State(n, E)
        s.boards[:], s.meta[:], s.legal[:] = b, m, all_legal(n, E)
        load(torch, env, s)
        ids = R.ids_from(id_base, E)
        env.sample_counter = counter
        assert env.sample_counter >= 2 ** 32
        acts, _, _ = env.sample_actions(logits)
        np.testing.assert_array_equal(acts.cpu().numpy(), R.sample_word(seed, ids, counter) >> shift)
        assert env.sample_counter == counter + 1
        acts = env.sample_step(logits)[0]
        np.testing.assert_array_equal(acts.cpu().numpy(), R.sample_word(seed, ids, counter + 1) >> shift)
        env.close()


# ------------------------------- (b) opening-length known answers, per kernel family
@pytest.mark.parametrize("ply", PLIES64)
@pytest.mark.parametrize("n", [6, 8, 10])
def test_opening_length_of_every_resetting_kernel(torch_cuda, n, ply):
    torch = torch_cuda
    E, seed = E_RAGGED, GOLDEN
    ids = R.ids_from(0, E)
    env = make_env(torch, E, n, sd=True, auto=True, seed=seed, init_rand=K)
    hole = one_empty_square(n, E)
    zeros = torch.zeros(E, dtype=torch.int32, device="cuda:0")
    want_reset = R.opening_len(seed, ids, ply, R.P_RESET, K)
    want_auto = R.opening_len(seed, ids, ply, R.P_AUTO, K)
    assert len(set(want_reset.tolist())) == 6 and len(set(want_auto.tolist())) == 6
    assert (want_reset != want_auto).any()
    what = "%dx%d ply %#x: " % (n, n, ply)

    # oth_reset (purpose 2; it reads the counter and leaves it), unmasked and masked
    env.ply_counter = ply
    env.reset()
    assert env.ply_counter == ply
    assert_start_with(env, want_reset, what + "oth_reset")
    load(torch, env, hole)
    mask = np.arange(E) % 3 == 1
    env.reset(mask=torch.from_numpy(mask))
    assert_start_with(env, want_reset[mask], what + "oth_reset masked", rows=mask)
    b, m, lg = get_state_np(env)
    assert (b[~mask] == hole.boards[0]).all() and (m[~mask] == 0).all() and (lg[~mask] == hole.legal[0]).all()

    # oth_step (purpose 1): action 0 is illegal at the start; sudden death ends every game
    env.reset()
    _, _, dones, _ = env.step(zeros, observe=False)
    assert bool(dones.all()) and env.ply_counter == ply + 1
    assert_start_with(env, want_auto, what + "oth_step")

    # from the one-empty-square position: every family plays square 0 and auto-resets
    def from_hole(name, run):
        load(torch, env, hole)
        env.ply_counter = ply
        acts, dones = run()
        assert env.ply_counter == ply + 1
        assert (acts.cpu().numpy().ravel() == 0).all(), what + name + ": square 0 not played"
        assert bool(dones.bool().all()), what + name + ": a game did not end"
        assert_start_with(env, want_auto, what + name)

    def policy(name):
        a, _, d = env.step_policy(name, n_plies=1)
        return a, d

    def sampled():
        out = env.sample_step(torch.randn(E, n * n, device="cuda:0"))
        return out[0], out[4]

    def observed():
        obs, _, d, _ = env.step(zeros, observe=True)
        np.testing.assert_array_equal(obs.cpu().numpy(), np.broadcast_to(start_obs, (E, n, n)))
        return zeros, d

    start_obs = oracle.observe(oracle.reset(n, 1))[0][0].astype(np.int64)
    from_hole("oth_step_policy random", lambda: policy("random"))
    from_hole("oth_step_policy greedy", lambda: policy("greedy"))
    from_hole("oth_sample_step", sampled)
    from_hole("oth_step_observe", observed)
    env.close()


@pytest.mark.parametrize("ply", PLIES64)
def test_opening_length_of_the_vs_kernels(torch_cuda, ply):
    """oth_reset_vs / oth_step_vs at 8x8: the draws take the call counter c as
    their ply (purpose 2 in the reset, 1 in a step's auto-reset), the opponent's
    moves ply c * 256 + j.  The device equals the oracle's turn loop, and the
    opening lengths equal rng_ref's."""
    torch = torch_cuda
    n, E, seed = 8, E_RAGGED, GOLDEN
    ids = R.ids_from(0, E)
    prot = np.where(np.arange(E) % 3 == 0, -1, 1).astype(np.int8)
    env = make_env(torch, E, n, sd=True, auto=True, seed=seed, init_rand=K)
    env.ply_counter = ply
    env.reset_vs("random", protagonist=torch.from_numpy(prot))
    assert env.ply_counter == ply + 1
    s = oracle.reset_vs(n, E, SD_AUTO, 0, ply, seed=seed, initial_rand_steps=K, prot=prot)
    b, m, lg = get_state_np(env)
    np.testing.assert_array_equal(b, s.boards)
    np.testing.assert_array_equal(m, s.meta)
    np.testing.assert_array_equal(lg, s.legal)
    np.testing.assert_array_equal(m >> 8, R.opening_len(seed, ids, ply, R.P_RESET, K))
    # a white protagonist's board: black (the opponent) has replied with the random move of ply c * 256
    white = prot == 1
    black_discs = np.bitwise_count(b[white, 0]) if hasattr(np, "bitwise_count") else \
        np.array([bin(int(v)).count("1") for v in b[white, 0]])
    assert (black_discs == 4).all()
    moved = b[white, 0] | b[white, 1]
    want_sq = start_moves(n)[R.scale_index(R.action_word(seed, ids[white], ply * 256), 4)]
    assert ((moved >> want_sq.astype(np.uint64)) & np.uint64(1)).all()

    s = one_empty_square(n, E)
    load(torch, env, s)
    env.ply_counter = ply
    acts = np.zeros(E, dtype=np.int32)
    orw, od, opl = oracle.step_vs(s, SD_AUTO, 0, ply, acts, seed=seed, initial_rand_steps=K, prot=prot)
    _, rew, dn, plies = env.step_vs(torch.from_numpy(acts).cuda(), "random", observe=False)
    np.testing.assert_array_equal(rew.cpu().numpy(), orw)
    np.testing.assert_array_equal(dn.cpu().numpy().view(np.uint8), od)
    np.testing.assert_array_equal(plies.cpu().numpy(), opl)
    assert od.all() and (opl == 1).all()
    b, m, lg = get_state_np(env)
    np.testing.assert_array_equal(b, s.boards)
    np.testing.assert_array_equal(m, s.meta)
    np.testing.assert_array_equal(lg, s.legal)
    np.testing.assert_array_equal(m >> 8, R.opening_len(seed, ids, ply, R.P_AUTO, K))
    env.close()


# ------------------------------------------------- (c) 64-bit replays on the oracle
@pytest.mark.parametrize("ply0", [2 ** 32 - 5, 2 ** 34 - 5])
@pytest.mark.parametrize("id_base", [2 ** 32 - 4096, 2 ** 32 - 1000])
@pytest.mark.parametrize("n,policy,init_rand", [(6, "random", 0), (8, "random", 0), (10, "random", 0),
                                                (8, "greedy", K)])
def test_replay_across_the_counter_carries(torch_cuda, n, policy, init_rand, id_base, ply0):
    """12 plies from ply counter 2^32 - 5 (the counter's low word carries) and
    2^34 - 5 (the Philox block counter's low word carries), ids up to 2^32 - 1 and
    wrapping past it, in one launch and split 5 + 7: identical to the oracle."""
    torch = torch_cuda
    E, plies, seed = 4096, 12, GOLDEN
    s = oracle.reset_openings(n, E, seed, id_base, ply0, init_rand) if init_rand else oracle.reset(n, E)
    oa, orw, od, owdl = oracle.rollout(s, SD_AUTO, 0 if policy == "random" else 1, plies, seed=seed,
                                       id_base=id_base, ply0=ply0, initial_rand_steps=init_rand)
    for split in ((12,), (5, 7)):
        env = make_env(torch, E, n, sd=True, auto=True, seed=seed, id_base=id_base, init_rand=init_rand)
        env.ply_counter = ply0
        env.reset()
        outs = [env.step_policy(policy, n_plies=k) for k in split]
        assert env.ply_counter == ply0 + plies
        acts, rews, dones = (torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(3))
        what = "%s %dx%d split %s" % (policy, n, n, split)
        np.testing.assert_array_equal(acts, oa, what)
        np.testing.assert_array_equal(rews, orw, what)
        np.testing.assert_array_equal(dones, od, what)
        b, m, lg = get_state_np(env)
        np.testing.assert_array_equal(b, s.boards, what)
        np.testing.assert_array_equal(m, s.meta, what)
        np.testing.assert_array_equal(lg, s.legal, what)
        np.testing.assert_array_equal(env.counts().cpu().numpy(), owdl, what)
        env.close()


# ------------------------------------------------------------------ (d) sensitivity
def device_random_actions(torch, seed, id_base, ply0, plies=4, E=4096):
    env = make_env(torch, E, 8, sd=True, auto=True, seed=seed, id_base=id_base)
    env.ply_counter = ply0
    acts = env.step_policy("random", n_plies=plies)[0].cpu().numpy()
    env.close()
    return acts


def device_reset_lengths(torch, seed, id_base, ply0, E=4096):
    env = make_env(torch, E, 8, sd=True, auto=True, seed=seed, id_base=id_base, init_rand=K)
    env.ply_counter = ply0
    env.reset()
    m = get_state_np(env)[1]
    env.close()
    return m >> 8


@pytest.mark.parametrize("a,b", SENSITIVITY_PAIRS)
def test_actions_depend_on_every_key_bit(torch_cuda, a, b):
    """A truncation shared with the oracle would pass every parity test: runs that
    differ only in an upper seed bit, an upper counter bit or the id base must
    differ in more than half of their actions."""
    x, y = device_random_actions(torch_cuda, *a), device_random_actions(torch_cuda, *b)
    assert (x != y).mean() > 0.5, (x != y).mean()


@pytest.mark.parametrize("a,b", SENSITIVITY_PAIRS[:3])
def test_reset_lengths_depend_on_upper_key_bits(torch_cuda, a, b):
    x, y = device_reset_lengths(torch_cuda, *a), device_reset_lengths(torch_cuda, *b)
    assert (x != y).mean() > 0.5, (x != y).mean()


# ------------------------------------- (e) statistics of the device's own output
class EnvCache(object):
    """One 65,536-board 8x8 env per (seed, initial_rand_steps)."""

    def __init__(self, torch):
        self.torch, self.envs = torch, {}

    def get(self, seed, init_rand):
        key = (seed, init_rand)
        if key not in self.envs:
            self.envs[key] = make_env(self.torch, STAT_E, 8, sd=True, auto=True, seed=seed, init_rand=init_rand)
        return self.envs[key]

    def close(self):
        for e in self.envs.values():
            e.close()


def test_opening_length_statistics_of_the_device(torch_cuda):
    """test_rng_spec_cpu's families on the lengths oth_reset (purpose 2) and
    oth_step_policy's auto-reset (purpose 1) return.  Successive resets of one
    env (ply+1, ply+2) are successive one-ply oth_step_policy calls, the
    one-empty-square position reloaded in between."""
    torch = torch_cuda
    cache = EnvCache(torch)
    hole = one_empty_square(8, STAT_E)

    def draw(seed, ply, purpose):
        env = cache.get(seed, K)
        if env.ply_counter != ply:  # a successive draw finds the counter where the last call left it
            env.ply_counter = ply
        if purpose == R.P_RESET:
            env.reset()
        else:
            load(torch, env, hole)
            env.step_policy("random", n_plies=1, record=False)
            assert env.ply_counter == ply + 1
        got = get_state_np(env)[1] >> 8
        np.testing.assert_array_equal(got, R.opening_len(seed, STAT_IDS, ply, purpose, K))
        return got

    worst = opening_families(draw)
    cache.close()
    check_bounds(worst, OPENING_BOUNDS, "device opening lengths")


def test_move_pick_statistics_of_the_device(torch_cuda):
    """The random policy's pick among the start position's four moves, and among
    the three replies, from two plies of oth_step_policy at 65,536 boards."""
    torch = torch_cuda
    cache = EnvCache(torch)
    first_moves = start_moves(8)
    s = oracle.reset(8, 4)
    oracle.step(s, SD_AUTO, first_moves.astype(np.int32))
    replies = np.array([[a for a in range(64) if (int(s.legal[i, 0]) >> a) & 1] for i in range(4)])
    assert replies.shape == (4, 3)

    def draw(seed, ply0):
        env = cache.get(seed, 0)
        env.reset()
        env.ply_counter = ply0
        acts = env.step_policy("random", n_plies=2)[0].cpu().numpy()
        first = np.searchsorted(first_moves, acts[0])
        assert (first_moves[np.minimum(first, 3)] == acts[0]).all(), "a first move outside the four legal ones"
        hit = replies[first] == acts[1][:, None]
        assert hit.any(1).all(), "a reply outside the three legal ones"
        reply = hit.argmax(1)
        np.testing.assert_array_equal(first, R.scale_index(R.action_word(seed, STAT_IDS, ply0), 4))
        np.testing.assert_array_equal(reply, R.scale_index(R.action_word(seed, STAT_IDS, ply0 + 1), 3))
        return first, reply

    worst = pick_families(draw)
    cache.close()
    check_bounds(worst, PICK_BOUNDS, "device move picks")
