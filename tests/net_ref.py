"""The network of include/othello_mi355x.h (oth_net_blob_bytes / oth_net_pack /
oth_net_eval) in numpy int64 and plain Python integers: rows in the exchange
format in; logits, priors and values out.  No float takes part but in the EXP2
list, which the header fixes by its formula."""
import numpy as np

EXP2 = [round(2 ** 30 * 2.0 ** (-f / 256)) for f in range(256)]
BIAS_MAX = 1 << 30


def nwords(n):
    return (n * n + 63) // 64


def bits(words, nn):
    """uint64 (R, W) -> int64 (R, nn): bit a of a row's words."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    a = np.arange(nn)
    return ((words[:, a >> 6] >> (a & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int64)


def features(n, boards, meta, legal):
    """int64 (R, 3 nn): the mover's bits, the opponent's, the legal bits."""
    nn, W = n * n, nwords(n)
    boards = np.asarray(boards, dtype=np.uint64).reshape(-1, 2 * W)
    white = (np.asarray(meta).astype(np.int64) & 1).astype(bool)[:, None]
    black_w, white_w = boards[:, :W], boards[:, W:]
    mover = np.where(white, white_w, black_w)
    opp = np.where(white, black_w, white_w)
    return np.concatenate([bits(mover, nn), bits(opp, nn), bits(np.asarray(legal).reshape(-1, W), nn)], axis=1)


class Net(object):
    """weights: L + 1 int8 arrays (H, F), (H, H) .., (nn + 1, H); biases: L + 1 int32 arrays."""

    def __init__(self, n, weights, biases, shifts, policy_shift, value_shift):
        self.n, self.nn = n, n * n
        self.w = [np.asarray(w).astype(np.int64) for w in weights]
        self.b = [np.asarray(b).astype(np.int64) for b in biases]
        self.L, self.H = len(self.w) - 1, self.w[0].shape[0]
        self.shifts, self.policy_shift, self.value_shift = [int(s) for s in shifts], int(policy_shift), int(value_shift)
        assert len(self.shifts) == self.L and 1 <= self.L <= 4 and self.H % 64 == 0 and 64 <= self.H <= 512
        assert self.w[0].shape == (self.H, 3 * self.nn) and self.w[-1].shape == (self.nn + 1, self.H)
        assert all(abs(b).max() <= BIAS_MAX for b in self.b)

    def logits(self, boards, meta, legal):
        h = features(self.n, boards, meta, legal)
        for l in range(self.L):
            acc = h @ self.w[l].T + self.b[l]
            assert abs(acc).max() < 2 ** 31
            h = np.clip(acc >> self.shifts[l], 0, 127)
        z = h @ self.w[-1].T + self.b[-1]
        assert abs(z).max() < 2 ** 31
        return z

    def evaluate(self, boards, meta, legal):
        """-> (priors int32 (R, nn), values int32 (R,), logits int32 (R, nn + 1))."""
        z = self.logits(boards, meta, legal)
        R, nn = z.shape[0], self.nn
        values = np.clip(z[:, nn] >> self.value_shift, -32768, 32768).astype(np.int32)
        lg = bits(np.asarray(legal).reshape(R, -1), nn)
        priors = np.zeros((R, nn), dtype=np.int32)
        for r in range(R):
            M = [a for a in range(nn) if lg[r, a]]
            if not M:
                continue
            m = max(int(z[r, a]) for a in M)
            e = {}
            for a in M:
                d = (m - int(z[r, a])) >> self.policy_shift
                i, f = d >> 8, d & 255
                e[a] = 0 if i >= 31 else EXP2[f] >> i
            S = sum(e.values())
            assert S >= 2 ** 30
            for a in M:
                priors[r, a] = (65535 * e[a] + S // 2) // S
        return priors, values, z.astype(np.int32)
