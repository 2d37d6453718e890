"""The cases of oth_puct_noise that the host build (tests/test_noise_host.py) and the
device (tests/test_gpu_noise.py) are held to, with what tests/noise_ref.py makes of
them.  A case is synthetic on purpose: the call reads the handle's boards and stored
possible_moves as words, so the words need not be positions of a game, and rows with
no, one and many legal squares, masks with bits off the board, leaves of every kind
and leaf boards that differ from the handle's in one bit of any word are all there at
every size."""
import collections

import numpy as np

import noise_ref as nf

E = 70
SIZES = (4, 6, 8, 10, 13, 16)  # W = 1, 1, 1, 2, 3, 4
EPSILONS = (0, 1, 64, 256)
SEED = 0xFEDCBA9876543210
TABLE_KEYS = [(n, K, mode, inplace) for n in SIZES for K in (1, 3) for mode in ("root", "leaf")
              for inplace in (False, True)]
TABLE_IDS = ["n%d-K%d-%s-%s" % (n, K, mode, "inplace" if ip else "out") for n, K, mode, ip in TABLE_KEYS]

Case = collections.namedtuple("Case", ("n", "K", "handle_boards", "handle_legal", "kind", "boards", "priors", "table",
                                       "seed", "id_key", "id_base", "counter"))


def synthetic_table(gen):
    """Monotone, a run of zeros at the bottom, the top entry 2^24 - 1: the shape of a gamma table."""
    t = np.sort(gen.integers(0, 1 << 24, nf.TABLE, dtype=np.int64))
    t[:400] = 0
    t[-1] = (1 << 24) - 1
    return t.astype(np.uint32)


def board_mask(n):
    nn, W = n * n, nf.nwords(n)
    m = np.zeros(W, dtype=np.uint64)
    for a in range(nn):
        m[a // 64] |= np.uint64(1) << np.uint64(a % 64)
    return m


def make(n, K, mode, table=None, id_key=0, id_base=0, counter=5, salt=0):
    """One case: E boards, K rows a board; mode "root" or "leaf"."""
    gen = np.random.default_rng([n, K, mode == "leaf", salt])
    nn, W = n * n, nf.nwords(n)
    full = board_mask(n)
    hb = gen.integers(0, 2 ** 63, (E, 2 * W), dtype=np.uint64) & np.tile(full, 2)
    hl = np.zeros((E, W), dtype=np.uint64)
    for e in range(E):
        if e % 5 == 0:
            continue  # no legal square
        if e % 5 == 1:
            a = int(gen.integers(0, nn))  # one
            hl[e, a // 64] = np.uint64(1) << np.uint64(a % 64)
        elif e % 5 == 2:
            hl[e] = full  # every square
        else:
            hl[e] = gen.integers(0, 2 ** 63, W, dtype=np.uint64) & gen.integers(0, 2 ** 63, W, dtype=np.uint64) & full
        if e % 3 == 0:
            hl[e] |= ~full  # bits off the board, which the call must not read as squares
    kind = boards = None
    if mode == "leaf":
        kind = gen.integers(0, 4, E * K).astype(np.uint8)
        boards = gen.integers(0, 2 ** 63, (E * K, 2 * W), dtype=np.uint64)
        for e in range(E):
            r = e * K
            kind[r] = (1, 1, 1, 0, 2, 3, 1)[e % 7]  # mostly EXPAND, and every other kind
            boards[r] = hb[e]
            if e % 11 == 4:  # another position: one bit of one word differs
                j = (e // 11) % (2 * W)
                boards[r, j] ^= np.uint64(1) << np.uint64(e % 64)
            for j in range(1, K):  # a later row is never the board's row, whatever it holds
                kind[r + j] = 1
                boards[r + j] = hb[e]
    priors = gen.integers(-3000, 70000, (E * K, nn)).astype(np.int32)
    priors[::4, :] = np.clip(priors[::4, :], 0, 65535)
    if table is None:
        table = synthetic_table(gen)
    return Case(n, K, hb, hl, kind, boards, priors, table, SEED, id_key, id_base, counter)


def expected(c, epsilon):
    """(the output, the applied boards) by the reference."""
    return nf.noise(c.n, c.handle_boards, c.handle_legal, c.priors, epsilon, c.table, c.seed, c.id_key, c.id_base,
                    c.counter, c.K, c.kind, c.boards)


def check_coverage(c, epsilon, want, applied):
    """The case exercises what it is there for."""
    nn = c.n * c.n
    counts = [len(nf.legal_squares(c.handle_legal[e], nn)) for e in range(E)]
    assert 0 in counts and 1 in counts and max(counts) > 4
    assert (c.priors < 0).any() and (c.priors > 65535).any()
    if c.kind is None:
        assert applied.all()
    else:
        first = c.kind[::c.K]
        assert set(first.tolist()) == {0, 1, 2, 3} and 0 < applied.sum() < (first == 1).sum()
    rows = np.arange(E) * c.K
    changed = (want[rows] != c.priors[rows]).any(1)
    assert not changed[~applied].any()
    if epsilon > 0 and c.table.any():
        assert changed[applied].any()
    others = np.setdiff1d(np.arange(E * c.K), rows)
    assert (want[others] == c.priors[others]).all()


# the special cases: (name, make's keywords)
BIG = np.full(nf.TABLE, 1 << 24, dtype=np.uint32)
BIG[1::3] = (1 << 24) + 12345
BIG[2::3] = 0x80000005  # negative as an int32
BIG[::64] = 7
SPECIAL = [
    ("counter-max", dict(n=8, K=1, mode="root", counter=2 ** 64 - 1)),
    ("counter-max-leaf", dict(n=10, K=3, mode="leaf", counter=2 ** 64 - 1)),
    ("id-wraps", dict(n=8, K=1, mode="root", id_key=2 ** 32 - 7, id_base=0)),
    ("id-base-wraps", dict(n=13, K=1, mode="root", id_key=5, id_base=2 ** 32 - 40)),
    ("zero-table", dict(n=8, K=3, mode="leaf", table=np.zeros(nf.TABLE, dtype=np.uint32))),
    ("clamped-table", dict(n=8, K=1, mode="root", table=BIG)),
    ("clamped-table-16", dict(n=16, K=1, mode="root", table=BIG)),
]
SPECIAL_IDS = [name for name, _ in SPECIAL]
