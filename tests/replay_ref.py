"""The replay store of include/othello_mi355x.h (oth_replay_begin / _append /
_label / _counts / _gather / _sample, oth_symmetry_masks) in plain Python
integers -- TEST REFERENCE ONLY.  Written from the header's comment; it calls no
project code but tests/rng_ref.py for the Philox block of the sample's draw.  A
board is one Python int per colour (bit a = square a), a row a small dict."""
import numpy as np

import rng_ref as rng

EMPTY, OPEN, LABELLED = 0, 1, 2
VISITS_MAX, OUTCOME_MAX = 2 ** 24 - 1, 32768
P_REPLAY = 5  # the Philox purpose word of the sample's draw
NAMES = ("state", "boards", "meta", "legal", "visits", "outcome", "rows", "sym")


def nwords(n):
    return (n * n + 63) // 64


def to_int(words):
    return sum(int(w) << (64 * j) for j, w in enumerate(words))


def to_words(x, W):
    return [(x >> (64 * j)) & (2 ** 64 - 1) for j in range(W)]


def sigma(n, s, a):
    """The square that stored square a goes to under symmetry s."""
    r, c = divmod(a, n)
    if s & 1:
        r, c = c, r
    if s & 2:
        r = n - 1 - r
    if s & 4:
        c = n - 1 - c
    return r * n + c


def permutations(n):
    """(8, N*N): [s][a] = sigma_s(a)."""
    return np.array([[sigma(n, s, a) for a in range(n * n)] for s in range(8)], dtype=np.int64)


_TABLES = {}


def table(n):
    """permutations(n) as lists, made once a size."""
    if n not in _TABLES:
        _TABLES[n] = permutations(n).tolist()
    return _TABLES[n]


def transform(n, s, x):
    """The mask x (a Python int) under symmetry s; squares off the board are dropped."""
    out, to = 0, table(n)[s]
    for a in range(n * n):
        if (x >> a) & 1:
            out |= 1 << to[a]
    return out


def symmetry_masks(n, sym, arr):
    """oth_symmetry_masks: arr uint64 (cnt, planes, W), sym (cnt,)."""
    W = nwords(n)
    out = np.zeros_like(arr)
    for i in range(arr.shape[0]):
        for p in range(arr.shape[1]):
            out[i, p] = to_words(transform(n, int(sym[i]) & 7, to_int(arr[i, p])), W)
    return out


def _mix(h):
    h &= 2 ** 64 - 1
    h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    return h ^ (h >> 31)


def synthetic_visits(E, move, nn):
    """The tests' visit counts: an integer hash of (e, move, square) on every square, the mask's or
    not, with negatives and values above 2^24; every seventh (board, move) has no positive count."""
    out = np.zeros((E, nn), dtype=np.int32)
    for e in range(E):
        quiet = (e + move) % 7 == 3
        for a in range(nn):
            h = _mix((e * 1000003 + move) * 7919 + a + 1)
            out[e, a] = -(h % 5) if quiet else h % 41 - 8 + (2 ** 25 if h % 13 == 0 else 0)
    return out


class Batch(object):
    def __init__(self, n, cnt):
        W, nn = nwords(n), n * n
        self.state = np.zeros(cnt, dtype=np.uint8)
        self.boards = np.zeros((cnt, 2 * W), dtype=np.uint64)
        self.meta = np.zeros(cnt, dtype=np.uint16)
        self.legal = np.zeros((cnt, W), dtype=np.uint64)
        self.visits = np.zeros((cnt, nn), dtype=np.int32)
        self.outcome = np.zeros(cnt, dtype=np.int32)
        self.rows = np.zeros(cnt, dtype=np.int32)
        self.sym = np.zeros(cnt, dtype=np.uint8)

    def arrays(self):
        return tuple(getattr(self, k) for k in NAMES)


class Store(object):
    """oth_replay_begin's store of E boards of size n with H slots a board."""

    def __init__(self, n, E, H):
        self.n, self.E, self.H, self.W, self.nn = n, E, H, nwords(n), n * n
        self.rows = [dict(state=EMPTY) for _ in range(E * H)]
        self.count, self.span, self.last_turn = [0] * E, [0] * E, [0] * E

    def append(self, s, visits, skip=None):
        """s: the handle's state (boards, meta, legal in exchange format); visits (E, N*N)."""
        W, board = self.W, (1 << self.nn) - 1
        recorded = 0
        for e in range(self.E):
            meta = int(s.meta[e])
            self.last_turn[e] = meta & 1
            stored = to_int(s.legal[e])
            c = [min(max(int(visits[e][a]), 0), VISITS_MAX) if (stored & board) >> a & 1 else 0 for a in range(self.nn)]
            if meta & 2 or (skip is not None and int(skip[e]) != 0) or sum(c) <= 0:
                continue
            self.rows[e * self.H + self.count[e] % self.H] = dict(
                state=OPEN, black=to_int(s.boards[e][:W]), white=to_int(s.boards[e][W:]), legal=stored, turn=meta & 1,
                visits=c, outcome=0)
            self.count[e] += 1
            self.span[e] = min(self.span[e] + 1, self.H)
            recorded += 1
        return recorded

    def label(self, rewards, dones):
        for e in range(self.E):
            if int(dones[e]) == 0:
                continue
            z = min(max(int(rewards[e]), -OUTCOME_MAX), OUTCOME_MAX)
            for k in range(self.span[e]):
                row = self.rows[e * self.H + (self.count[e] - 1 - k) % self.H]
                if row["state"] == OPEN:
                    row["state"] = LABELLED
                    row["outcome"] = z if row["turn"] == self.last_turn[e] else -z
            self.span[e] = 0

    def counts(self):
        st = [r["state"] for r in self.rows]
        return np.array([st.count(EMPTY), st.count(OPEN), st.count(LABELLED)], dtype=np.int64)

    def _emit(self, b, i, row, s):
        n, W = self.n, self.W
        b.rows[i] = row if 0 <= row < len(self.rows) else -1
        b.sym[i] = s
        r = self.rows[row] if 0 <= row < len(self.rows) else dict(state=EMPTY)
        if r["state"] == EMPTY:
            return  # zeros everywhere
        b.state[i] = r["state"]
        b.boards[i] = to_words(transform(n, s, r["black"]), W) + to_words(transform(n, s, r["white"]), W)
        b.legal[i] = to_words(transform(n, s, r["legal"]), W)
        b.meta[i] = r["turn"]
        b.outcome[i] = r["outcome"]
        b.visits[i, table(n)[s]] = r["visits"]

    def gather(self, rows, sym=None):
        b = Batch(self.n, len(rows))
        for i, row in enumerate(rows):
            self._emit(b, i, int(row), 0 if sym is None else int(sym[i]) & 7)
        return b

    def sample_rows(self, cnt, augment, seed, id_key, counter):
        """The rows and symmetries oth_replay_sample draws."""
        labelled = [j for j, r in enumerate(self.rows) if r["state"] == LABELLED]
        M = len(labelled)
        ids = (int(id_key) + np.arange(cnt, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
        u = rng.philox4x32_10(seed, ids, counter, P_REPLAY)
        rows = [labelled[(int(u[i, 0]) * M) >> 32] if M else -1 for i in range(cnt)]
        sym = [int(u[i, 1]) >> 29 if augment else 0 for i in range(cnt)]
        return rows, sym

    def sample(self, cnt, augment, seed, id_key, counter):
        rows, sym = self.sample_rows(cnt, augment, seed, id_key, counter)
        b = Batch(self.n, cnt)
        for i in range(cnt):
            self._emit(b, i, rows[i], sym[i])
        return b

    def all_rows(self):
        return np.arange(self.E * self.H, dtype=np.int32)
