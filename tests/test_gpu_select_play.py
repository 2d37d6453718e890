"""The play kernels' pick without compares and selects (select64_tab by sign
masks and the rank-reversed sel8 table; select_bit_tab on two-word boards) on
the device, bit for bit against the oracle's replay: 1,000 boards (15 full
waves and a partial one of 40 lanes, three full blocks and a partial one) x 130
plies from the start position with auto-reset, seed 5 -- 8x8 and 6x6 random play
(k_play_rand<N, random>), 8x8 greedy play after random openings of up to 10
plies (k_play_rand<8, greedy>) and 10x10 random play (k_play_rand_w<10>), each
with win/loss and with disk-difference rewards, once as one launch and once as
launches of 1, 2, 3, 5, 8, ... plies (most of them starting inside a Philox
group).  Actions, rewards, dones, the final state and the W/D/L tally."""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

E = 1000
PLIES = 130
SEED = 5
CONFIGS = {
    "random8": (8, "random", 0),
    "random6": (6, "random", 0),
    "greedy8_open10": (8, "greedy", 10),
    "random10": (10, "random", 0),
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def flags_of(disk):
    return oracle.F_SUDDEN_DEATH | oracle.F_AUTO_RESET | (oracle.F_DISK_REWARD if disk else 0)


def start(n, init_rand):
    return oracle.reset_openings(n, E, SEED, 0, 0, init_rand) if init_rand else oracle.reset(n, E)


def launches():
    """1, 2, 3, 5, 8, ... plies per launch, the last one what is left of PLIES."""
    parts, a, b = [], 1, 2
    while sum(parts) + a < PLIES:
        parts.append(a)
        a, b = b, a + b
    return parts + [PLIES - sum(parts)]


_TURNS, _REF = {}, {}


def turns(cfg):
    """The side to move at the start of every ply and after the last, and the
    dones, from the oracle's replay one ply at a time (once per configuration;
    board ranges on host threads, as oracle.rollout_parallel)."""
    if cfg not in _TURNS:
        import concurrent.futures
        n, policy, init_rand = CONFIGS[cfg]
        pid = 0 if policy == "random" else 1
        t = start(n, init_rand)
        turn = np.zeros((PLIES + 1, E), dtype=np.uint16)
        dones = np.zeros((PLIES, E), dtype=np.uint8)
        T = 8
        cuts = [E * k // T for k in range(T + 1)]

        def part(k):
            lo, hi = cuts[k], cuts[k + 1]
            sub = oracle.State(n, hi - lo)
            sub.boards[:], sub.meta[:], sub.legal[:] = t.boards[lo:hi], t.meta[lo:hi], t.legal[lo:hi]
            turn[0, lo:hi] = sub.meta & 1
            for p in range(PLIES):
                _, _, d1, _ = oracle.rollout(sub, flags_of(False), pid, 1, seed=SEED, id_base=lo, ply0=p,
                                             initial_rand_steps=init_rand)
                turn[p + 1, lo:hi] = sub.meta & 1
                dones[p, lo:hi] = d1[0]

        with concurrent.futures.ThreadPoolExecutor(T) as ex:
            list(ex.map(part, range(T)))
        _TURNS[cfg] = (turn, dones)
    return _TURNS[cfg]


def reference(cfg, disk):
    """The oracle's replay of PLIES plies in one call (once per configuration and reward kind)."""
    if (cfg, disk) not in _REF:
        n, policy, init_rand = CONFIGS[cfg]
        s = start(n, init_rand)
        oa, orw, od, owdl = oracle.rollout_parallel(s, flags_of(disk), 0 if policy == "random" else 1, PLIES,
                                                    seed=SEED, initial_rand_steps=init_rand)
        _REF[(cfg, disk)] = (oa, orw, od, owdl, s)
    return _REF[(cfg, disk)]


def check_against(env, got, ref):
    oa, orw, od, owdl, s = ref
    acts, rews, dones = (x.cpu().numpy() for x in got)
    np.testing.assert_array_equal(acts, oa)
    np.testing.assert_array_equal(rews, orw)
    np.testing.assert_array_equal(dones, od)
    b, m, lg = env.get_state()
    np.testing.assert_array_equal(b.cpu().numpy().view(np.uint64), s.boards)
    np.testing.assert_array_equal(m.cpu().numpy().view(np.uint16), s.meta)
    np.testing.assert_array_equal(lg.cpu().numpy().view(np.uint64), s.legal)  # possible_moves
    np.testing.assert_array_equal(env.counts().cpu().numpy(), owdl)


@pytest.mark.parametrize("disk", [False, True], ids=["winloss", "disks"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_play_one_launch_and_split(torch_cuda, cfg, disk):
    torch = torch_cuda
    from gymothelloenv_amd import VecOthelloEnv
    n, policy, init_rand = CONFIGS[cfg]
    ref = reference(cfg, disk)
    # what the replay itself must contain: game ends, and passes (a ply that ends no
    # game and leaves the turn where it was)
    turn, dones1 = turns(cfg)
    np.testing.assert_array_equal(dones1, ref[2])
    ends = int((ref[2] != 0).sum())
    passes = int(((turn[1:] == turn[:-1]) & (ref[2] == 0)).sum())
    print("%s: %d game ends, %d passes in %d board-plies" % (cfg, ends, passes, E * PLIES))
    assert ends >= 1000 and passes >= 100, (ends, passes)
    if disk:  # disk-difference rewards differ from the win/loss ones somewhere
        assert not np.array_equal(ref[1], reference(cfg, False)[1])

    def make():
        env = VecOthelloEnv(E, board_size=n, auto_reset=True, num_disk_as_reward=disk, seed=SEED,
                            initial_rand_steps=init_rand, device="cuda:0")
        env.reset()
        return env

    one = make()
    check_against(one, one.step_policy(policy, n_plies=PLIES), ref)
    one.close()
    split = make()
    parts = [split.step_policy(policy, n_plies=k) for k in launches()]
    check_against(split, tuple(torch.cat([p[i] for p in parts]) for i in range(3)), ref)
    split.close()
