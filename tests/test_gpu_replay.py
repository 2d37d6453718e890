"""oth_replay_begin / _append / _label / _counts / _gather / _sample, oth_symmetry_masks
and VecOthelloEnv's replay methods on the device against the plain Python integers of
tests/replay_ref.py: whole games of env.step on random legal actions with synthetic
visits, the store read back through gather after every call.  Every comparison is
exact equality."""
import numpy as np
import pytest

import replay_cases as rc
import replay_ref as rr
from oracle import oracle
from test_gpu_puct import make_env, state_np, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

VIEWS = dict(boards=np.uint64, meta=np.uint16, legal=np.uint64)


def dev(torch, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def batch_np(batch):
    """A ReplayBatch as numpy arrays in replay_ref.NAMES' order (None where the field was not made)."""
    out = []
    for k in rr.NAMES:
        t = getattr(batch, k)
        out.append(None if t is None else t.cpu().numpy().view(VIEWS.get(k, t.cpu().numpy().dtype)))
    return out


class DeviceStore(object):
    """The env's replay methods behind the interface replay_cases drives."""

    def __init__(self, torch, env, H, B):
        self.torch, self.env = torch, env
        env.replay_begin(H, B)
        env._replay_ws.fill_(0xA5)  # the workspace starts as garbage
        env.replay_begin(H, B)

    def append(self, s, visits, skip=None):
        self.env.replay_append(dev(self.torch, visits), None if skip is None else dev(self.torch, skip))

    def label(self, rewards, dones):
        self.env.replay_label(dev(self.torch, np.asarray(rewards, dtype=np.int32)),
                              dev(self.torch, np.asarray(dones, dtype=np.uint8)))

    def counts(self):
        return self.env.replay_counts().cpu().numpy()

    def gather(self, rows, sym=None, **kw):
        kw.setdefault("layout", None)
        return batch_np(self.env.replay_gather(dev(self.torch, rows), None if sym is None else dev(self.torch, sym),
                                               **kw))

    def sample(self, n, augment, seed, id_key, counter, **kw):
        kw.setdefault("layout", None)
        return batch_np(self.env.replay_sample(n, augment, seed=seed, counter=counter, id_key=id_key, **kw))


class EnvGame(object):
    """Boards stepped on the device: the reference is fed with the handle's own state."""

    def __init__(self, torch, env):
        self.torch, self.env = torch, env

    def state(self):
        s = oracle.State(self.env.board_size, self.env.num_envs)
        s.boards[:], s.meta[:], s.legal[:] = state_np(self.env)
        return s

    def step(self, actions):
        _, rewards, dones, _ = self.env.step(dev(self.torch, actions), observe=False)
        return rewards.cpu().numpy(), dones.cpu().numpy().astype(np.uint8)


def played(torch, n, E, H, B, auto_reset, disk_reward, moves, every, what):
    """A store after `moves` plies of play, held against the reference after every call."""
    env = make_env(E, n, seed=5, auto_reset=auto_reset, num_disk_as_reward=disk_reward)
    ds, ref = DeviceStore(torch, env, H, B), rr.Store(n, E, H)
    rc.check_store(ds, ref, what + " begin")
    tally = rc.play(ds, ref, EnvGame(torch, env), moves, 17, what, every)
    return env, ds, ref, tally


# (n, E, H, auto_reset, disk_reward): W = 1, 1, 2, 3, 4 words (81 squares straddle a word); H = 3 wraps a
# game's ring many times; 37 x 31 = 1,147 rows cross the 1,024-row chunk of the rank step
CASES = [(4, 5, 3, False, False), (4, 5, 3, True, True), (8, 5, 3, True, False), (8, 5, 3, False, True),
         (9, 5, 3, False, False), (9, 5, 3, True, True), (12, 5, 3, True, False), (12, 5, 3, False, True),
         (16, 5, 3, False, False), (16, 5, 3, True, True), (4, 37, 31, True, True), (8, 37, 31, False, False),
         (9, 37, 31, True, False)]
CASE_ID = "n%d-E%d-H%d-auto%d-disk%d"


@pytest.mark.parametrize("c", CASES, ids=lambda c: CASE_ID % c)
def test_games_against_the_reference(torch_cuda, c):
    """Games played to the end (every square but the first four can take a disc: N*N - 4 plies at the most,
    a few more label boards that are done and have no record)."""
    n, E, H, auto_reset, disk_reward = c
    nn = n * n
    env, ds, ref, (recorded, finished, labelled) = played(torch_cuda, n, E, H, E * H + 4, auto_reset, disk_reward,
                                                          nn - 2, 32 if E * H > 100 or n > 9 else 4, CASE_ID % c)
    assert recorded > E and finished >= E and labelled > 0
    if not auto_reset:
        assert (state_np(env)[1] & 2).all(), "a game did not end"
    if H == 3:
        assert max(ref.count) > 2 * H, "the ring did not wrap"
    # a label with dones all 0 changes nothing
    before = env._replay_ws.clone()
    ds.label(np.full(E, 5, dtype=np.int32), np.zeros(E, dtype=np.uint8))
    assert torch_cuda.equal(env._replay_ws, before)
    env.close()


@pytest.mark.parametrize("n", [8, 9])
def test_gather_under_every_symmetry_with_obs(torch_cuda, n):
    """Every row under all eight symmetries, obs in make_state / float32 and board / int8 against oth_observe
    of a second handle set to the gathered arrays; and fields left out of the batch change nothing else."""
    torch = torch_cuda
    E, H = 5, 3
    R = E * H + 1
    env, ds, ref, _ = played(torch, n, E, H, 8 * R, True, False, 12, 12, "gather")
    rows = np.tile(np.arange(R, dtype=np.int32), 8)
    sym = np.repeat(np.arange(8, dtype=np.uint8), R)
    want = ref.gather(rows, sym)
    assert (want.state == rr.OPEN).any() and (want.state == rr.EMPTY).any()
    other = make_env(rows.size, n)
    for layout, dtype in (("make_state", torch.float32), ("board", torch.int8)):
        b = env.replay_gather(dev(torch, rows), dev(torch, sym), layout=layout, dtype=dtype)
        rc.same_batch(batch_np(b), want.arrays(), "gather %s" % layout)
        other.set_state(b.boards, b.meta, b.legal)
        assert torch.equal(b.obs, other.observe(layout, dtype))
        # the same obs through the staging rows: the batch without boards, meta and legal
        narrow = env.replay_gather(dev(torch, rows), dev(torch, sym), layout=layout, dtype=dtype,
                                   fields=("obs", "outcome"))
        assert narrow.boards is None and narrow.visits is None and torch.equal(narrow.obs, b.obs)
        assert torch.equal(narrow.outcome, b.outcome)
    only = ds.gather(rows, sym, fields=("visits", "sym"))
    rc.same_batch(only, want.arrays(), "visits and sym alone")
    assert only[0] is None and only[4] is not None
    rc.same_batch(ds.gather(rows), ref.gather(rows).arrays(), "sym NULL")
    other.close()
    env.close()


def test_sample(torch_cuda):
    """M = 0, M = 1, and M over both chunks of the rank step with and without the symmetries; a captured
    sample replayed twice gives the same bytes; the call counter moves on."""
    torch = torch_cuda
    n, E, H, B = 4, 37, 31, 300  # B: the rows of a sample here; the store takes whole dumps too
    env = make_env(E, n, seed=5, auto_reset=True)
    ds, ref = DeviceStore(torch, env, H, E * H + 4), rr.Store(n, E, H)
    rc.same_batch(ds.sample(B, 1, 3, 4, 5), ref.sample(B, 1, 3, 4, 5).arrays(), "M = 0")
    assert (ds.sample(7, 1, 3, 4, 5)[6] == -1).all()
    visits = np.zeros((E, n * n), dtype=np.int32)
    visits[36] = 3  # only the last board records: row 36 * 31 = 1116, in the second chunk
    game = EnvGame(torch, env)
    for impl in (ds, ref):
        impl.append(game.state(), visits)
        impl.label(np.full(E, -2 ** 20, dtype=np.int32), np.ones(E, dtype=np.uint8))
    np.testing.assert_array_equal(ds.counts(), [E * H - 1, 0, 1])
    got = ds.sample(B, 1, 3, 4, 5)
    rc.same_batch(got, ref.sample(B, 1, 3, 4, 5).arrays(), "M = 1")
    assert (got[6] == 36 * H).all() and (got[5] == -32768).all() and len(set(got[7].tolist())) == 8
    rc.play(ds, ref, game, 30, 23, "sample", every=30)
    lab = [j for j, r in enumerate(ref.rows) if r["state"] == rr.LABELLED]
    assert min(lab) < 1024 <= max(lab) and len(lab) > 200
    for augment, seed, id_key, counter in ((1, 99, 0, 0), (0, 2 ** 64 - 1, 2 ** 32 - 3, 2 ** 63 + 5),
                                           (1, 7, 9, 2 ** 64 - 1)):
        want = ref.sample(B, augment, seed, id_key, counter)
        rc.same_batch(ds.sample(B, augment, seed, id_key, counter), want.arrays(), "sample")
        assert min(want.rows) < 1024 <= max(want.rows)
        assert len(set(want.sym.tolist())) == (8 if augment else 1)
        rc.same_batch(ds.sample(B, augment, seed, id_key, counter, fields=("outcome", "rows")), want.arrays(),
                      "sample, two fields")
    b = env.replay_sample(B, layout="make_state")
    other = make_env(B, n)
    other.set_state(b.boards, b.meta, b.legal)
    assert torch.equal(b.obs, other.observe("make_state", torch.float32)) and (b.state == rr.LABELLED).all()
    other.close()
    # the env's own key and counter
    env.replay_sample_counter = 40
    key = (env.seed ^ 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
    rc.same_batch(batch_np(env.replay_sample(B, layout=None)), ref.sample(B, 1, key, 0, 40).arrays(), "own counter")
    assert env.replay_sample_counter == 41
    # a capture records only; two replays give the same bytes, those of the eager call
    eager = [t.clone() for t in env.replay_sample(B, seed=1, counter=2) if t is not None]
    ws = env._replay_ws.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = [t for t in env.replay_sample(B, seed=1, counter=2) if t is not None]
    g.replay()
    torch.cuda.synchronize()
    first = [t.clone() for t in out]
    for t in out:
        t.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    assert len(out) == len(eager) == 9
    for x, y, z in zip(out, first, eager):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert torch.equal(env._replay_ws, ws)
    env.close()


def test_another_geometry_does_nothing(torch_cuda):
    """The same memory named with another max_batch: append, label, counts, gather and sample write nothing."""
    torch = torch_cuda
    n, E, H, B = 8, 5, 3, 32
    env, ds, ref, _ = played(torch, n, E, H, B, True, False, 6, 6, "geometry")
    before = env._replay_ws.clone()
    env._replay = (H, B - 1)
    ds.append(None, np.ones((E, n * n), dtype=np.int32))
    ds.label(np.ones(E, dtype=np.int32), np.ones(E, dtype=np.uint8))
    env.replay_counts()
    env.replay_gather(dev(torch, np.arange(4, dtype=np.int32)))
    env.replay_sample(4)
    assert torch.equal(env._replay_ws, before)
    env._replay = (H, B)
    rc.check_store(ds, ref, "afterwards")
    env.close()


@pytest.mark.parametrize("n", list(range(4, 17)))
def test_symmetry_masks_against_the_reference(torch_cuda, n):
    import gymothelloenv_amd as g
    torch = torch_cuda
    gen = np.random.default_rng(n)
    arr = gen.integers(0, 2 ** 64, size=(70, 3, rr.nwords(n)), dtype=np.uint64)  # more than one block of lanes
    sym = (np.arange(70) % 8 + 8 * (np.arange(70) % 3)).astype(np.uint8)
    got = g.symmetry_masks(n, dev(torch, sym), dev(torch, arr.view(np.int64)))
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64), rr.symmetry_masks(n, sym, arr))
    flat = g.symmetry_masks(n, dev(torch, sym), dev(torch, arr[:, 0].view(np.int64)))  # (n, W): one plane
    np.testing.assert_array_equal(flat.cpu().numpy().view(np.uint64), rr.symmetry_masks(n, sym, arr[:, :1])[:, 0])


def test_puct_play_records(torch_cuda):
    """puct_play(record=True) over a full 4 x 4 game of 4 boards with the uniform evaluator: the store equals
    the reference fed with the PuctPlay tuples; record=False leaves the counts as they are."""
    import gymothelloenv_amd as g
    torch = torch_cuda
    n, E, H = 4, 4, 16
    env = make_env(E, n, seed=2)
    ds, ref = DeviceStore(torch, env, H, E * H + 4), rr.Store(n, E, H)
    game = EnvGame(torch, env)
    for m in range(n * n):
        s = game.state()
        if (s.meta & 2).all():
            break
        mv = env.puct_play(g.uniform_evaluator, 12, record=True)
        ref.append(s, mv.visits.cpu().numpy())
        ref.label(mv.rewards.cpu().numpy(), mv.dones.cpu().numpy())
        rc.check_store(ds, ref, "move %d" % m, m)
    assert (game.state().meta & 2).all() and m > 4
    counts = ref.counts()
    assert counts[1] == 0 and counts[2] >= 4 * 5, "every record of the finished games is labelled"
    b = ds.gather(ref.all_rows())
    assert set(np.abs(b[5][b[0] == rr.LABELLED]).tolist()) <= {0, 1}
    env.reset()
    env.puct_begin()
    env.puct_play(g.uniform_evaluator, 12)
    env.puct_play(g.uniform_evaluator, 12, record=False)
    np.testing.assert_array_equal(ds.counts(), counts)
    env.close()
