"""The convolutional network of include/othello_mi355x.h (oth_cnet_blob_bytes /
oth_cnet_pack / oth_cnet_eval) in numpy int64 and plain Python integers: rows in the
exchange format in; logits, priors and values out.  The features, the bits and the
integer softmax are tests/net_ref.py's.

A conv's products are summed by a float64 matrix product where exact=False (the
default: every partial sum is an integer below 2^31, far inside float64's 2^53, so
the result is the int64 sum bit for bit; tests/test_cnet_census_cpu.py holds it
against exact=True, the einsum in int64, on a case)."""
import numpy as np

import net_ref as nr

BIAS_MAX = nr.BIAS_MAX
HEAD_OUT = 16


def conv(w, b, x, exact=False):
    """w int64 (O, I, 3, 3), b int64 (O,), x int64 (R, I, n, n) -> int64 (R, O, n, n); 0 off the board."""
    R, I, n, _ = x.shape
    O = w.shape[0]
    pad = np.zeros((R, I, n + 2, n + 2), dtype=np.int64)
    pad[:, :, 1:-1, 1:-1] = x
    acc = np.zeros((R, O, n, n), dtype=np.int64) + b[None, :, None, None]
    for ky in range(3):
        for kx in range(3):
            win = pad[:, :, ky:ky + n, kx:kx + n]
            if exact:
                acc += np.einsum("oi,riyx->royx", w[:, :, ky, kx], win)
            else:
                cols = win.transpose(1, 0, 2, 3).reshape(I, R * n * n).astype(np.float64)
                part = w[:, :, ky, kx].astype(np.float64) @ cols
                acc += part.astype(np.int64).reshape(O, R, n, n).transpose(1, 0, 2, 3)
    assert abs(acc - b[None, :, None, None]).max() < 2 ** 25 and abs(acc).max() < 2 ** 31
    return acc


def clip(v):
    return np.clip(v, 0, 127)


class ConvNet(object):
    """weights: the stem (C, 3, 3, 3), 2 B convs (C, C, 3, 3), the head (16, C, 3, 3), wv (nn, 15); biases: (C,),
    2 B of (C,), (16,), (1,)."""

    def __init__(self, n, weights, biases, shift_stem, shifts, shift_head, policy_shift, value_shift, exact=False):
        self.n, self.nn, self.exact = n, n * n, exact
        self.w = [np.asarray(w).astype(np.int64) for w in weights]
        self.b = [np.asarray(b).astype(np.int64) for b in biases]
        self.C, self.B = self.w[0].shape[0], len(shifts) // 2
        self.shift_stem, self.shifts, self.shift_head = int(shift_stem), [int(s) for s in shifts], int(shift_head)
        self.policy_shift, self.value_shift = int(policy_shift), int(value_shift)
        assert self.C in (64, 128) and 1 <= self.B <= 8 and len(self.shifts) == 2 * self.B
        assert len(self.w) == 2 * self.B + 3 and len(self.b) == 2 * self.B + 3
        assert self.w[0].shape == (self.C, 3, 3, 3) and self.w[-2].shape == (HEAD_OUT, self.C, 3, 3)
        assert self.w[-1].shape == (self.nn, 15) and self.b[-1].shape == (1,)
        assert all(0 <= s <= 24 for s in self.shifts + [self.shift_stem, self.shift_head, self.policy_shift,
                                                        self.value_shift])
        assert all(abs(b).max() <= BIAS_MAX for b in self.b)

    def planes(self, boards, meta, legal):
        x = nr.features(self.n, boards, meta, legal)
        return x.reshape(x.shape[0], 3, self.n, self.n)

    def layers(self, boards, meta, legal):
        """The accumulators and activations of every layer, in order: [(name, acc, act)], then the head's u."""
        out = []
        acc = conv(self.w[0], self.b[0], self.planes(boards, meta, legal), self.exact)
        h = clip(acc >> self.shift_stem)
        out.append(("stem", acc, h))
        for k in range(self.B):
            acc = conv(self.w[1 + 2 * k], self.b[1 + 2 * k], h, self.exact)
            t = clip(acc >> self.shifts[2 * k])
            out.append(("conv%d" % (2 * k), acc, t))
            acc = conv(self.w[2 + 2 * k], self.b[2 + 2 * k], t, self.exact)
            h = clip((acc >> self.shifts[2 * k + 1]) + h)
            out.append(("conv%d" % (2 * k + 1), acc, h))
        u = conv(self.w[-2], self.b[-2], h, self.exact)
        return out, u

    def logits(self, boards, meta, legal):
        """int64 (R, nn + 1): z_0 .. z_{nn - 1}, z_v."""
        _, u = self.layers(boards, meta, legal)
        R = u.shape[0]
        f = clip(u[:, 1:] >> self.shift_head).reshape(R, 15, self.nn)
        terms = np.einsum("aj,rja->r", self.w[-1], f)
        assert abs(terms).max() < 2 ** 26
        zv = self.b[-1][0] + terms
        assert abs(zv).max() < 2 ** 31
        return np.concatenate([u[:, 0].reshape(R, self.nn), zv[:, None]], axis=1)

    def evaluate(self, boards, meta, legal):
        """-> (priors int32 (R, nn), values int32 (R,), logits int32 (R, nn + 1))."""
        return softmax(self.logits(boards, meta, legal), legal, self.nn, self.policy_shift, self.value_shift)


class _Head(object):
    """What net_ref.Net.evaluate reads of its net: the logits and the two shifts."""

    def __init__(self, z, nn, policy_shift, value_shift):
        self.z, self.nn, self.policy_shift, self.value_shift = z, nn, policy_shift, value_shift

    def logits(self, boards, meta, legal):
        return self.z


def softmax(z, legal, nn, policy_shift, value_shift):
    """net_ref.Net.evaluate's head on these logits: the value and the integer softmax over the legal squares."""
    return nr.Net.evaluate(_Head(z, nn, policy_shift, value_shift), None, None, legal)
