"""The random draws' specification, pinned on the CPU: tests/rng_ref.py (an
independent numpy statement) against the published Philox4x32-10 known answers,
the host build of csrc/bitboard.hpp and the CPU oracle over full-width keys
(64-bit seeds and counters, 32-bit env ids), then the statistics of the draws
themselves: opening lengths and random-move picks are uniform and independent
across neighbouring env ids, plies, purposes and seeds.

The statistics run on fixed inputs, so each bound is a condition, not a flaky
test: a statistic must stay below the chi-square quantile at p = 1e-4
(rng_ref.CHI2_P1E4).  tests/test_gpu_rng.py runs the same families on what the
kernels return (opening_families / pick_families below take the draw as a
function)."""
import numpy as np
import pytest

import rng_ref as R
from oracle import oracle
from test_bitboard_host import hostlib, ptr  # noqa: F401

GOLDEN = 0x9E3779B97F4A7C15
SEEDS = (5, GOLDEN, 1 << 32)
COUNTERS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 34 - 1, (5 << 40) + 3)
SD_AUTO = oracle.F_SUDDEN_DEATH | oracle.F_AUTO_RESET
K = 10  # initial_rand_steps of the opening-length cases: six lengths 0, 2, .., 10

# statistics: inputs
STAT_E = 65536
STAT_SEEDS = (5, GOLDEN)
STAT_PLIES = (0, 2 ** 32 - 1, (5 << 40) + 3)
PICK_SEEDS = (0, 5, GOLDEN, 1 << 32)
PICK_PLIES = (0, 1, 2, 3, 2 ** 32 - 2, 2 ** 34 - 1, (5 << 40) + 1)
# statistics: bounds (chi-square quantile at p = 1e-4) and, next to each, the worst
# value measured on rng_ref over the inputs above / on the device's output (MI355X)
OPENING_BOUNDS = {
    "uniform": (5, 25.74),        # worst 7.44 / 7.44
    "id+1": (25, 60.14),          # worst 33.52 / 33.52
    "id+64": (25, 60.14),         # worst 35.24 / 35.24
    "ply+1": (25, 60.14),         # worst 38.87 / 38.87
    "ply+2": (25, 60.14),         # worst 41.48 / 41.48
    "purpose": (25, 60.14),       # worst 34.45 / 34.45
    "seed+1": (25, 60.14),        # worst 32.55 / 32.55
    "seed^bit32": (25, 60.14),    # worst 44.39 / 44.39
}
PICK_BOUNDS = {
    "uniform": (3, 21.11),        # worst 10.43 / 10.43
    "id+1": (9, 33.72),           # worst 16.80 / 16.80
    "reply|first": (2, 18.42),    # worst 9.41 / 9.41 (df 2: the quantile is -2 ln 1e-4)
}
for _b in list(OPENING_BOUNDS.values()) + list(PICK_BOUNDS.values()):
    assert _b[1] == R.CHI2_P1E4[_b[0]]


# ------------------------------------------------------------- known answers
KAT = [  # Random123 kat_vectors, philox4x32 10: counter, key, output
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    # (third word a20bc7c6, not ..c9 as sometimes quoted: torch's header-only
    # at::Philox4_32 and a plain-int restatement both give c6)
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


def test_reference_philox_known_answers():
    for ctr, key, want in KAT:
        got = [int(w[0]) for w in R.philox4x32_10_raw(ctr, key)]
        assert got == want, [hex(v) for v in got]
        # the same vectors through the (seed, id, ctr, purpose) layout
        blk = R.philox4x32_10(key[0] | key[1] << 32, [ctr[0]], ctr[1] | ctr[2] << 32, ctr[3])
        assert blk[0].tolist() == want


def test_host_build_philox_known_answers(hostlib):
    out = np.zeros(4, dtype=np.uint32)
    for ctr, key, want in KAT:
        hostlib.host_philox4(key[0] | key[1] << 32, ctr[0], ctr[1] | ctr[2] << 32, ctr[3], ptr(out))
        assert out.tolist() == want, [hex(v) for v in out]


def full_width_tuples(n, rs):
    """n random (seed u64, id u32, ctr u64, purpose u32) tuples, every field over
    its full width, the first few pinned to the corners."""
    def u64():
        return (rs.randint(0, 2 ** 32, size=n, dtype=np.uint64) << np.uint64(32)) | \
            rs.randint(0, 2 ** 32, size=n, dtype=np.uint64)
    seed, ctr = u64(), u64()
    ids = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    purpose = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    purpose[: n // 2] &= 3  # half of them the purposes in use
    top = np.uint64(2 ** 64 - 1)
    seed[:4] = [0, top, 1 << 32, 2 ** 32 - 1]
    ctr[:4] = [top, 0, 2 ** 32 - 1, 1 << 32]
    ids[:4] = [2 ** 32 - 1, 0, 2 ** 32 - 1, 1 << 31]
    return seed, ids, ctr, purpose


def test_host_build_matches_reference_over_full_width_keys(hostlib):
    """philox4, action_draw, opening_draw and scale_index of csrc/bitboard.hpp (the
    host build of the code the kernels run) == rng_ref on 10,000 random tuples."""
    n = 10000
    seed, ids, ctr, purpose = full_width_tuples(n, np.random.RandomState(2024))
    assert (seed >> np.uint64(32)).any() and (ctr >> np.uint64(32)).any() and (ids >> 31).any()
    want = R.philox4x32_10(seed, ids, ctr, purpose)
    got = np.zeros(4, dtype=np.uint32)
    for i in range(n):
        hostlib.host_philox4(int(seed[i]), int(ids[i]), int(ctr[i]), int(purpose[i]), ptr(got))
        assert got.tolist() == want[i].tolist(), (i, hex(int(seed[i])), hex(int(ctr[i])))
    out = np.zeros(n, dtype=np.uint32)
    hostlib.host_action_draw(n, ptr(seed), ptr(ids), ptr(ctr), ptr(out))
    np.testing.assert_array_equal(out, R.action_word(seed, ids, ctr))
    hostlib.host_opening_draw(n, ptr(seed), ptr(ids), ptr(ctr), ptr(purpose), ptr(out))
    np.testing.assert_array_equal(out, R.opening_word(seed, ids, ctr, purpose))
    m = np.random.RandomState(7).randint(1, 257, size=n).astype(np.int32)
    u = want[:, 1].copy()
    u[:6] = [0, 1, 2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1, 2 ** 32 - 2]
    idx = np.zeros(n, dtype=np.int32)
    hostlib.host_scale_index(n, ptr(u), ptr(m), ptr(idx))
    np.testing.assert_array_equal(idx, R.scale_index(u, m))
    np.testing.assert_array_equal(idx, [int(a) * int(b) >> 32 for a, b in zip(u, m)])  # plain ints
    assert (idx >= 0).all() and (idx < m).all()


def test_reference_pieces_in_plain_ints():
    """rng_ref's vectorised forms against plain-int arithmetic on one tuple each."""
    M = 0xFFFFFFFF

    def fmix(h):
        h ^= h >> 16
        h = h * 0x85EBCA6B & M
        h ^= h >> 13
        h = h * 0xC2B2AE35 & M
        return h ^ h >> 16
    for seed in SEEDS:
        for ply in COUNTERS:
            for purpose in (1, 2):
                key = fmix((seed & M) ^ fmix((seed >> 32) ^ (purpose * 0x7FEB352D & M)))
                c = fmix(key ^ (ply & M) ^ ((ply >> 32) * 0x9E3779B9 & M))
                ids = [0, 1, 77, 2 ** 32 - 1]
                assert R.opening_word(seed, ids, ply, purpose).tolist() == [fmix(c ^ i) for i in ids]
            blk = R.philox4x32_10(seed, [9], ply >> 2, 0)
            assert int(R.action_word(seed, [9], ply)[0]) == int(blk[0, ply & 3])
            assert int(R.sample_word(seed, [9], ply)[0]) == int(R.philox4x32_10(seed, [9], ply, 3)[0, 0])


# ------------------------------------------------- the oracle against rng_ref
START_MOVES = {}


def start_moves(n):
    """The start position's legal squares, ascending (four on every board size)."""
    if n not in START_MOVES:
        lg = oracle.reset(n, 1).legal[0]
        START_MOVES[n] = np.array([a for a in range(n * n) if (int(lg[a // 64]) >> (a % 64)) & 1])
        assert len(START_MOVES[n]) == 4
    return START_MOVES[n]


def assert_start(s, what=""):
    """Every board of State s is the start position with black to move (meta's low byte 0)."""
    ref = oracle.reset(s.n, 1)
    assert (s.boards == ref.boards[0]).all(), what + ": not the start position"
    assert (s.legal == ref.legal[0]).all(), what + ": possible_moves are not the start position's"
    assert ((s.meta & 0xff) == 0).all(), what + ": turn / terminated / winner bits set"


@pytest.mark.parametrize("id_base", [0, 2 ** 32 - 1000])
@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_draws_match_reference(seed, id_base):
    """reset_openings (purpose 2), the auto-reset of step (purpose 1) and the random
    policy's move, on the grid of 64-bit seeds and counters; ids wrap past 2^32."""
    n, E = 8, 4096
    ids = R.ids_from(id_base, E)
    assert id_base == 0 or ids[-1] < ids[0]
    for ctr in COUNTERS:
        what = "seed %#x id_base %#x ctr %#x" % (seed, id_base, ctr)
        s = oracle.reset_openings(n, E, seed, id_base, ctr, K)
        np.testing.assert_array_equal(s.meta >> 8, R.opening_len(seed, ids, ctr, R.P_RESET, K), what)
        assert_start(s, what)
        # action 0 is illegal at the start: sudden death ends every game, auto-reset draws
        s = oracle.reset(n, E)
        _, dones, _ = oracle.step(s, SD_AUTO, np.zeros(E, dtype=np.int32), seed=seed, id_base=id_base, ply=ctr,
                                  initial_rand_steps=K)
        assert dones.all()
        np.testing.assert_array_equal(s.meta >> 8, R.opening_len(seed, ids, ctr, R.P_AUTO, K), what)
        assert_start(s, what)
        s = oracle.reset(n, E)
        acts, _, _, _ = oracle.rollout(s, SD_AUTO, 0, 1, seed=seed, id_base=id_base, ply0=ctr)
        np.testing.assert_array_equal(acts[0], start_moves(n)[R.scale_index(R.action_word(seed, ids, ctr), 4)], what)


def oracle_random_actions(n, E, seed, id_base, ply0, plies=4):
    s = oracle.reset(n, E)
    return oracle.rollout(s, SD_AUTO, 0, plies, seed=seed, id_base=id_base, ply0=ply0)[0]


SENSITIVITY_PAIRS = [  # (seed, id_base, ply0) twice: the two runs must differ
    ((7, 0, 0), (7 | 1 << 32, 0, 0)),
    ((7, 0, 0), (7 | 1 << 63, 0, 0)),
    ((7, 0, 0), (7, 0, 2 ** 34)),
    ((7, 0, 0), (7, 2 ** 20, 0)),
]


@pytest.mark.parametrize("a,b", SENSITIVITY_PAIRS)
def test_oracle_actions_depend_on_every_key_bit(a, b):
    """Four plies of random play at 4,096 boards: runs that differ only in an upper
    seed bit, an upper counter bit or the id base differ in more than half of
    their actions (independent uniform picks among 3-6 moves agree ~ 1 in 4)."""
    x, y = oracle_random_actions(8, 4096, *a), oracle_random_actions(8, 4096, *b)
    assert (x != y).mean() > 0.5, (x != y).mean()


@pytest.mark.parametrize("a,b", SENSITIVITY_PAIRS[:3])
def test_oracle_opening_lengths_depend_on_upper_key_bits(a, b):
    """The same for reset()'s opening lengths (six lengths: independent draws agree 1 in 6)."""
    x = oracle.reset_openings(8, 4096, a[0], a[1], a[2], K).meta >> 8
    y = oracle.reset_openings(8, 4096, b[0], b[1], b[2], K).meta >> 8
    assert (x != y).mean() > 0.5, (x != y).mean()


# ------------------------------------------------------- statistics of the spec
def opening_families(draw, seeds=STAT_SEEDS, plies=STAT_PLIES, n_len=K // 2 + 1):
    """Worst chi-square statistic per family of OPENING_BOUNDS.  draw(seed, ply,
    purpose) -> the opening lengths (0, 2, .., K) of STAT_E consecutive env ids
    from 0; results are cached per key, so a neighbour's draw is made once."""
    cache = {}

    def get(seed, ply, purpose):
        key = (seed, ply, purpose)
        if key not in cache:
            x = np.asarray(draw(seed, ply, purpose)).astype(np.int64)
            assert x.shape == (STAT_E,) and (x % 2 == 0).all() and x.min() >= 0 and x.max() <= 2 * (n_len - 1)
            cache[key] = x // 2
        return cache[key]

    worst = {f: 0.0 for f in OPENING_BOUNDS}
    for seed in seeds:
        for ply in plies:
            for purpose in (R.P_AUTO, R.P_RESET):
                x = get(seed, ply, purpose)
                pairs = {
                    "id+1": (x[:-1], x[1:]),
                    "id+64": (x[:-64], x[64:]),
                    "ply+1": (x, get(seed, ply + 1, purpose)),
                    "ply+2": (x, get(seed, ply + 2, purpose)),
                    "purpose": (x, get(seed, ply, 3 - purpose)),
                    "seed+1": (x, get(seed + 1, ply, purpose)),
                    "seed^bit32": (x, get(seed ^ (1 << 32), ply, purpose)),
                }
                worst["uniform"] = max(worst["uniform"], R.chi2_uniform(x, n_len))
                for f, (a, b) in pairs.items():
                    worst[f] = max(worst[f], R.chi2_table(a, b, n_len, n_len))
    return worst


def pick_families(draw, seeds=PICK_SEEDS, plies=PICK_PLIES):
    """Worst chi-square statistic per family of PICK_BOUNDS.  draw(seed, ply0) ->
    (first, reply): the index among the start position's four moves picked at ply0
    and the index among the three replies picked at ply0 + 1, for STAT_E
    consecutive env ids from 0."""
    worst = {f: 0.0 for f in PICK_BOUNDS}
    for seed in seeds:
        for ply0 in plies:
            first, reply = (np.asarray(v).astype(np.int64) for v in draw(seed, ply0))
            assert first.shape == reply.shape == (STAT_E,)
            worst["uniform"] = max(worst["uniform"], R.chi2_uniform(first, 4))
            worst["id+1"] = max(worst["id+1"], R.chi2_table(first[:-1], first[1:], 4, 4))
            for m in range(4):
                worst["reply|first"] = max(worst["reply|first"], R.chi2_uniform(reply[first == m], 3))
    return worst


def check_bounds(worst, bounds, who):
    print("%s worst chi-square per family: %s" % (who, ", ".join("%s %.2f" % kv for kv in sorted(worst.items()))))
    for f, (df, bound) in bounds.items():
        assert worst[f] < bound, "%s: %s statistic %.2f >= %.2f (df %d, p = 1e-4)" % (who, f, worst[f], bound, df)


STAT_IDS = np.arange(STAT_E)


def test_opening_length_statistics_of_the_spec():
    worst = opening_families(lambda seed, ply, purpose: R.opening_len(seed, STAT_IDS, ply, purpose, K))
    check_bounds(worst, OPENING_BOUNDS, "rng_ref opening lengths")


def test_move_pick_statistics_of_the_spec():
    worst = pick_families(lambda seed, ply0: (R.scale_index(R.action_word(seed, STAT_IDS, ply0), 4),
                                              R.scale_index(R.action_word(seed, STAT_IDS, ply0 + 1), 3)))
    check_bounds(worst, PICK_BOUNDS, "rng_ref move picks")


def test_chi_square_helpers():
    """The helpers on tables worked by hand, and that they do flag a biased or a
    dependent draw of the size the bounds are meant to catch."""
    assert R.chi2_uniform([0, 0, 0, 1], 2) == pytest.approx(1.0)           # (3-2)^2/2 + (1-2)^2/2
    assert R.chi2_table([0, 0, 1, 1], [0, 0, 1, 1], 2, 2) == pytest.approx(4.0)  # n for a perfect 2x2 dependence
    assert R.chi2_table([0, 0, 1, 1], [0, 1, 0, 1], 2, 2) == pytest.approx(0.0)
    rs = np.random.RandomState(1)
    x = rs.randint(0, 6, size=STAT_E)
    assert R.chi2_uniform(x, 6) < 25.74 and R.chi2_table(x[:-1], x[1:], 6, 6) < 60.14
    biased = np.where(rs.rand(STAT_E) < 0.03, 0, x)        # 3 % of the draws forced to one length
    assert R.chi2_uniform(biased, 6) > 25.74
    sticky = np.where(rs.rand(STAT_E) < 0.05, np.roll(x, 1), x)  # 5 % of the draws repeat the neighbour's
    assert R.chi2_table(sticky[:-1], sticky[1:], 6, 6) > 60.14
