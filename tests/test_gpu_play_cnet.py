"""oth_play_cnet, oth_reset_vs_cnet and oth_step_vs_cnet on the device
(VecOthelloEnv.play_net, reset_vs / step_vs and NetPolicy with a NetPlayer of a
DeviceConvNet) against the reference loops of tests/play_net_ref.py over
tests/cnet_ref.ConvNet.  Every comparison is exact equality.

The shapes are the smallest that cross k_play_cnet's edges:
  N = 4   one square tile, four boards a workgroup (sides mixed within a round); E = 1, 3, 9
  N = 5   two boards a workgroup, a ragged second tile; E = 5
  N = 6   one board a workgroup, a ragged third tile; E = 9, C = 128, B = 2
  N = 8   four full tiles, a full word; E = 17; once C = 128, B = 2
  N = 10  two words, seven tiles (more than one pass of a wave's four); E = 5
  N = 16  four words, LDS above 64 KiB at C = 128; E = 2, at most 12 plies, once
4 x 4 and 5 x 5 run n^2 plies, so that games end (and reset) inside a run.

The conditions that make a comparison mean something are asserted on the reference's
output alone (play_cnet_cases.play_facts).  One of them, "at most half of the
network-chosen moves are the lowest legal square", is taken over the moves that had
a choice (two stored squares or more): a forced move says nothing about the logits,
and the late plies of a 4 x 4 game are mostly forced -- over all network-chosen
moves the reference's share is 0.44 .. 0.64 on 4 x 4 run to n^2 plies whatever the
weights, and 0.04 .. 0.37 from 5 x 5 up; over the moves with a choice it is at most
0.42 on 4 x 4.  The seed is one for which every condition holds on the reference."""
import ctypes

import numpy as np
import pytest

import net_ref as nr
import play_cnet_cases as pc
import play_net_ref as pn
from oracle import oracle

pytestmark = pytest.mark.gpu

FLAG_SETS = {0: {}, 3: dict(sudden_death_on_invalid_move=True, num_disk_as_reward=True), 4: dict(auto_reset=True)}
# (N, E, C, B)
PLAY_SHAPES = [(4, 1, 64, 1), (4, 3, 64, 1), (4, 9, 64, 1), (5, 5, 64, 1), (6, 9, 128, 2), (8, 17, 64, 1), (10, 5, 64, 1)]


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


_DEV = {}


def dev_net(n, B, C, salt=0):
    from gymothelloenv_amd.cnet import DeviceConvNet
    key = (n, B, C, salt)
    if key not in _DEV:
        _DEV[key] = DeviceConvNet(n, *pc.ref_net(*key)[1], device="cuda:0")
    return _DEV[key]


def both(n, B, C, salt=0):
    return pc.ref_net(n, B, C, salt)[0], dev_net(n, B, C, salt)


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


def plies_of(n):
    return n * n if n <= 5 else (12 if n == 16 else 2 * n * n // 3)


# ------------------------------------------------------------ 1. play mode equals the reference loop
def check_play(torch, n, E, black, white, flags, rand, plies, start=None, seed=13, id_base=1000):
    """black / white: ((reference net, device net), sample_discs).  -> (A, D, play_facts)"""
    from gymothelloenv_amd import NetPlayer
    env = make_env(E, n, flags, initial_rand_steps=rand, seed=seed, env_id_base=id_base)
    if start is not None:
        load(torch, env, start)
    s = state_of(env)
    first = s.copy()
    ply0 = env.ply_counter
    pb = NetPlayer(black[0][1], black[1])
    pw = None if white is black else NetPlayer(white[0][1], white[1])
    got = outputs(env.play_net(pb, pw, plies))
    rb, rw = (black[0][0], black[1]), (white[0][0], white[1])
    if white is black:
        rw = rb
    A, R, D, wdl, chose = pn.play(rb, rw, s, flags, plies, seed=seed, id_base=id_base, ply0=ply0, initial_rand_steps=rand)
    what = "n=%d E=%d flags=%d rand=%d sample_discs=%d/%d" % (n, E, flags, rand, black[1], white[1])
    assert chose[0] > 0 and chose[1] > 0, what  # by the reference alone: both colours' plies were the network's
    for name, g, w in zip(("actions", "rewards", "dones"), got, (A, R, D)):
        assert g.shape == (plies, E)
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (name, what))
    assert_state(env, s, what)
    np.testing.assert_array_equal(env.counts().cpu().numpy(), wdl, err_msg=what)
    assert env.ply_counter == ply0 + plies
    env.close()
    facts = pc.play_facts((rb[0], rw[0]), first, flags, A, seed, id_base, ply0, rand, (rb[1], rw[1]))
    assert facts[0] == chose[0] + chose[1]
    return A, D, facts


def one_net_cases(torch, n, E, C, B, flags, rand):
    """The three sample_discs settings of one (shape, flags, openings) with one network, and the conditions the
    reference's output has to meet for the comparison to mean something."""
    nets = both(n, B, C)
    assert pc.ref_net(n, B, C)[2] > 0.3  # the census: saturation hides nothing
    choice = lowest = ended = 0
    for sample_discs in (0, 257, n * n // 2):
        # from the reset board without openings or draws every board plays one game: those start from varied positions
        start = pc.varied(n, E, 4) if rand == 0 and sample_discs == 0 else None
        side = (nets, sample_discs)
        A, D, facts = check_play(torch, n, E, side, side, flags, rand, plies_of(n), start)
        choice, lowest, ended = choice + facts[1], lowest + facts[2], ended + int(D.sum())
        if sample_discs:
            assert facts[3], "a drawn move differs from the argmax of its position"
            if E > 1:
                assert len({tuple(A[:, e]) for e in range(E)}) == E, "the boards' games are pairwise distinct"
    assert 2 * lowest <= choice  # a kernel that ignores the logits cannot pass
    if n <= 5:
        assert ended > 0  # games end inside the run (and reset with flags 4)


@pytest.mark.parametrize("rand", [0, 6])
@pytest.mark.parametrize("flags", [0, 3, 4])
@pytest.mark.parametrize("n,E,C,B", PLAY_SHAPES, ids=["n%d-E%d-C%d-B%d" % s for s in PLAY_SHAPES])
def test_play_equals_the_reference(torch_cuda, n, E, C, B, flags, rand):
    one_net_cases(torch_cuda, n, E, C, B, flags, rand)


def test_play_8x8_128_channels(torch_cuda):
    nets = both(8, 2, 128)
    check_play(torch_cuda, 8, 17, (nets, 12), (nets, 12), 4, 6, 20)


def test_play_16x16_lds_above_64k(torch_cuda):
    nets = both(16, 1, 128)
    side = (nets, 257)
    A, _, facts = check_play(torch_cuda, 16, 2, side, side, 0, 0, plies_of(16))
    assert facts[3] and tuple(A[:, 0]) != tuple(A[:, 1])


# ------------------------------------------------------------ 2. two different networks
@pytest.mark.parametrize("n,E,C", [(4, 9, 64), (5, 5, 64), (8, 17, 64)])
def test_two_networks(torch_cuda, n, E, C):
    """Different weights, B = 1 against B = 2, different shifts; one on each colour and the pair swapped; the boards
    of a workgroup are at different plies, so that they want different sides in the same round."""
    a, b = both(n, 1, C), both(n, 2, C, salt={4: 3}.get(n, 1))  # (a draw whose fitted shifts differ from a's)
    assert ((a[0].shift_stem, a[0].shifts, a[0].shift_head, a[0].policy_shift) !=
            (b[0].shift_stem, b[0].shifts[:2], b[0].shift_head, b[0].policy_shift))
    start = pc.staggered(n, E)
    plies = 12
    runs = {}
    for name, (black, white) in {"ab": ((a, 0), (b, n * n // 2)), "ba": ((b, n * n // 2), (a, 0))}.items():
        A, _, facts = check_play(torch_cuda, n, E, black, white, 0, 0, plies, start, seed=21, id_base=5)
        runs[name] = A
        if pc.rows_per_block(n) > 1:
            assert facts[4], "two boards of one workgroup have different movers at some ply"
    # by the reference alone: the run tells the two networks apart
    same = pn.play((a[0], 0), (a[0], 0), start.copy(), 0, plies, seed=21, id_base=5)[0]
    assert (runs["ab"] != same).any() and (runs["ab"] != runs["ba"]).any()


def test_players_of_one_network_are_one_and_channel_counts_must_agree(torch_cuda):
    torch = torch_cuda
    from gymothelloenv_amd import NetPlayer
    n, E = 5, 5
    _, d64 = both(n, 1, 64)
    start = pc.staggered(n, E)
    res = []
    p = NetPlayer(d64, 9)
    for black, white in ((NetPlayer(d64, 9), None), (NetPlayer(d64, 9), NetPlayer(d64, 9)), (p, p)):
        env = make_env(E, n, 0, seed=21, env_id_base=5)
        load(torch, env, start)
        res.append(outputs(env.play_net(black, white, 8)) + list(state_np(env)))
        env.close()
    for other in res[1:]:
        for x, y in zip(res[0], other):
            np.testing.assert_array_equal(x, y)
    env = make_env(E, n)
    with pytest.raises(ValueError, match="same channels"):
        env.play_net(NetPlayer(d64), NetPlayer(dev_net(n, 1, 128)))
    env.close()


# ------------------------------------------------------------ 3. vs mode equals vs_reset / vs_calls
@pytest.mark.parametrize("n,E,C,B,sample_discs", [(4, 9, 64, 1, 257), (4, 9, 64, 1, 0), (5, 5, 64, 1, 257),
                                                   (8, 17, 64, 1, 0), (8, 17, 64, 1, 257), (10, 5, 64, 1, 257)])
def test_vs_equals_the_reference(torch_cuda, n, E, C, B, sample_discs):
    torch = torch_cuda
    from gymothelloenv_amd import NetPlayer
    net, dnet = both(n, B, C)
    prot = np.where(np.arange(E) % 3 == 0, -1, 1).astype(np.int8)
    mask = (np.arange(E) % 4 != 1).astype(np.uint8)
    flags, rand = 4, 6
    n_calls = 10 if n <= 5 else 3
    kw = dict(seed=7, id_base=300, initial_rand_steps=rand)
    what = "n=%d sample_discs=%d" % (n, sample_discs)
    env = make_env(E, n, flags, initial_rand_steps=rand, seed=7, env_id_base=300)
    env.ply_counter = 5
    player, opp = NetPlayer(dnet, sample_discs), (net, sample_discs)
    before = state_of(env)
    env.reset_vs(player, protagonist=torch.from_numpy(prot), mask=torch.from_numpy(mask))
    s = pn.vs_reset(opp, n, E, flags, prot, 5, into=before, mask=mask, **kw)
    assert_state(env, s, "after the masked reset_vs, " + what)
    env.reset_vs(player, protagonist=torch.from_numpy(prot))
    s = pn.vs_reset(opp, n, E, flags, prot, 6, **kw)
    assert_state(env, s, "after reset_vs, " + what)
    ref, wdl, vs = pn.vs_calls(opp, s, flags, prot, n_calls, call0=7, **kw)
    for c, (acts, r, d, plies, after) in enumerate(ref):
        assert env.ply_counter == 7 + c
        _, gr, gd, gp = env.step_vs(torch.from_numpy(acts).cuda(), player, protagonist=torch.from_numpy(prot),
                                    observe=False)
        for name, g, w in zip(("rewards", "dones", "plies"), outputs((gr, gd, gp)), (r, d, plies)):
            np.testing.assert_array_equal(g, w, err_msg="%s of call %d, %s" % (name, c, what))
        assert_state(env, after, "after call %d, %s" % (c, what))
    np.testing.assert_array_equal(env.counts().cpu().numpy(), wdl, err_msg=what)
    np.testing.assert_array_equal(env.counts_vs().cpu().numpy(), vs, err_msg=what)
    assert max(int(c[3].max()) for c in ref) >= 2  # the opponent replied
    if n <= 5:
        assert vs.sum() > 0  # games end, are tallied and reset with the opponent's replies
    env.close()


# ------------------------------------------------------------ 4. a wrong blob changes nothing
def test_mismatched_blob_changes_nothing(torch_cuda):
    torch = torch_cuda
    from gymothelloenv_amd import NetPlayer
    from gymothelloenv_amd.cnet import DeviceConvNet
    from gymothelloenv_amd.vec_env import _ptr
    n, E, C = 8, 17, 64
    w, b, ss, sh, shd, ps, vs = pc.ref_net(n, 1, C)[1]
    good = dev_net(n, 1, C)
    shifted = DeviceConvNet(n, w, b, ss, [sh[0], sh[1] + 1], shd, ps, vs, device="cuda:0")  # one block shift: a byte behind the tags
    deeper = dev_net(n, 2, C, salt=1)                                                        # another B: tag 0
    assert shifted.blob.numel() == good.blob.numel() < deeper.blob.numel()
    ok = NetPlayer(good, 0)
    env = make_env(E, n, 4, seed=3)
    env.step_policy("random", 50, record=False)
    torch.cuda.synchronize()
    before, counts, cvs, ply = state_np(env), env.counts().cpu().numpy(), env.counts_vs().cpu().numpy(), env.ply_counter
    lib, h, st = env._lib, env._h, env._stream()
    a, r = torch.full((2, E), 77, dtype=torch.int32).cuda(), torch.full((2, E), 77, dtype=torch.int32).cuda()
    d = torch.full((2, E), 77, dtype=torch.uint8).cuda()
    p1 = torch.full((E,), 77, dtype=torch.int32).cuda()
    acts = env.greedy_actions()
    g = ctypes.addressof(ok._struct)
    calls = 0
    for other in (shifted, deeper):
        bad = NetPlayer(good, 0)
        bad._struct.blob = other.blob.data_ptr()  # the params say one thing, the bytes another
        x = ctypes.addressof(bad._struct)
        assert lib.oth_play_cnet(h, x, x, 2, _ptr(a), _ptr(r), _ptr(d), st) == 0
        assert lib.oth_play_cnet(h, g, x, 2, _ptr(a), _ptr(r), _ptr(d), st) == 0
        assert lib.oth_play_cnet(h, x, g, 2, _ptr(a), _ptr(r), _ptr(d), st) == 0
        assert lib.oth_reset_vs_cnet(h, x, None, None, st) == 0
        assert lib.oth_step_vs_cnet(h, x, _ptr(acts), None, _ptr(r), _ptr(d), _ptr(p1), st) == 0
        calls += 8
        torch.cuda.synchronize()
    for t in (a, r, d, p1):
        assert (t == 77).all()
    for u, v in zip(before, state_np(env)):
        np.testing.assert_array_equal(u, v)
    np.testing.assert_array_equal(env.counts().cpu().numpy(), counts)
    np.testing.assert_array_equal(env.counts_vs().cpu().numpy(), cvs)
    assert env.ply_counter == ply + calls  # the ply counter has advanced all the same
    # and the right bytes play
    assert lib.oth_play_cnet(h, g, g, 2, _ptr(a), _ptr(r), _ptr(d), st) == 0
    torch.cuda.synchronize()
    assert (a != 77).all()
    env.close()


# ------------------------------------------------------------ 5. launch splits
def test_launch_splits(torch_cuda):
    from gymothelloenv_amd import NetPlayer
    n, E, P = 4, 9, 16
    player = NetPlayer(dev_net(n, 1, 64), 257)

    def run(split, E=E, base=0):
        env = make_env(E, n, 4, initial_rand_steps=6, seed=13, env_id_base=base)
        parts = [outputs(env.play_net(player, None, k)) for k in split]
        out = [np.concatenate([p[i] for p in parts]) for i in range(3)] + list(state_np(env)) + [env.counts().cpu().numpy()]
        env.close()
        return out

    whole = run([P])
    for split in ([1] * P, [5, 11]):
        for x, y in zip(whole, run(split)):
            np.testing.assert_array_equal(x, y)
    # two handles of half the boards: the global env id keys a draw
    E2 = 10
    whole, lo, hi = run([P], E2), run([P], E2 // 2, 0), run([P], E2 // 2, E2 // 2)
    for k in range(3):
        np.testing.assert_array_equal(whole[k], np.concatenate([lo[k], hi[k]], axis=1))
    for k in range(3, 6):
        np.testing.assert_array_equal(whole[k], np.concatenate([lo[k], hi[k]], axis=0))
    np.testing.assert_array_equal(whole[6], lo[6] + hi[6])
    assert whole[6].sum() > 0 and len({tuple(whole[0][:, e]) for e in range(E2)}) == E2
    assert (run([P], E2 // 2, 0)[0] != hi[0]).any()


# ------------------------------------------------------------ 6. capture in a graph region
@pytest.mark.parametrize("n,E,C,K", [(8, 17, 64, 3), (16, 2, 128, 2)])
def test_capture_in_a_graph_region(torch_cuda, n, E, C, K):
    """play_net(n_plies=K) with a conv NetPlayer captured on a side stream inside graph_region: replay r equals an
    eager twin's call at counter base + K r, with fresh draws per replay.  At N = 16, C = 128 the kernel's LDS
    attribute is set before the launch is recorded."""
    torch = torch_cuda
    from gymothelloenv_amd import NetPlayer
    player = NetPlayer(dev_net(n, 1, C), 257)
    kw = dict(initial_rand_steps=0 if n == 16 else 6, seed=9)
    env, twin = make_env(E, n, 4, **kw), make_env(E, n, 4, **kw)
    twin.ply_counter = 0
    sd = env.state_dict()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), env.graph_region() as slot:
        out = env.play_net(player, None, K)
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
        want = twin.play_net(player, None, K)
        for x, y in zip(out, want):
            assert torch.equal(x, y)
        for x, y in zip(env.get_state(), twin.get_state()):
            assert torch.equal(x, y)
        if prev is not None:
            assert not torch.equal(prev, out[0])  # fresh draws per replay
        prev = out[0].clone()
    assert env.ply_counter == 0 and env.graph_offsets(slot)[0] == 2 * K
    env.close()
    twin.close()


# ------------------------------------------------------------ 7. the drop-in env
def test_dropin_env_plays_the_reference_move(torch_cuda):
    import gymothelloenv_amd as g
    n = 6
    net, dnet = both(n, 1, 64)
    single = g.OthelloEnv(black_policy=g.NetPolicy(dnet), protagonist=g.WHITE_DISK, board_size=n, device="cuda:0")
    single.reset()
    prot, flags = np.array([1], np.int8), 1  # sudden death on an invalid move: OthelloEnv's default
    s = pn.vs_reset((net, 0), n, 1, flags, prot, 0)
    for step in range(5):
        moves = [int(a) for a in np.flatnonzero(nr.bits(s.legal, n * n)[0])]
        assert sorted(int(a) for a in single.possible_moves) == moves, "before step %d" % step
        a = moves[len(moves) // 2]
        _, reward, done, _ = single.step(a)
        (_, r, d, _, _), = pn.vs_calls((net, 0), s, flags, prot, 1, call0=1 + step, act=lambda st: np.array([a], np.int32))[0]
        assert (reward, bool(done)) == (int(r[0]), bool(d[0]))
        assert not done
    single.close()
