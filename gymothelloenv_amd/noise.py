"""Dirichlet root noise for self-play, drawn on the device in integers (oth_puct_noise;
include/othello_mi355x.h defines the draw and the mix).

    dirichlet_table   the gamma table of a concentration alpha: the one place where
                      floats appear, on the host, as quantize_module is for the weights
    RootNoise         (epsilon, alpha) as VecOthelloEnv.puct_search / puct_play take it
                      (`noise=`): round(256 epsilon) and the table

The draws themselves are VecOthelloEnv.puct_noise: keyed by (seed, global env id,
counter, square), so a self-play run with noise is still an exact function of the
boards, the parameters, the weight bytes and the seeds."""
import torch

from . import _lib as L

ALPHA_MIN, ALPHA_MAX = 0.01, 100.0


def gamma_quantiles(alpha, p):
    """The Gamma(alpha, 1) quantiles at the probabilities p (a float64 tensor in (0, 1)), by
    bisection on the regularised lower incomplete gamma function: float64, on the host."""
    a = torch.full_like(p, float(alpha))
    lo = torch.zeros_like(p)
    hi = torch.full_like(p, float(alpha) + 12.0 * float(alpha) ** 0.5 + 40.0)  # P(alpha, hi) is 1 to the last bit
    for _ in range(1200):  # until no double lies between: the quantiles of a small alpha go down to the denormals
        mid = 0.5 * (lo + hi)
        if bool(((mid == lo) | (mid == hi)).all()):
            break
        below = torch.special.gammainc(a, mid) < p
        lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
    return hi


def dirichlet_table(alpha, device=None):
    """oth_puct_noise's gamma table of a Dirichlet(alpha) noise: int32 (4096,), table[i]
    = round(q_i / q_4095 (2^24 - 1)), q_i the Gamma(alpha, 1) quantile at (i + 0.5) /
    4096.  A Dirichlet draw is a vector of independent gamma draws divided by their
    sum, which is scale-free, so normalising to the top entry spends the whole range
    of an entry.  alpha must lie in [0.01, 100] (ValueError otherwise).

    A very small alpha puts nearly all of a gamma draw's mass next to zero: most
    entries of the table are then 0 (alpha = 0.03: about six in ten), a row whose
    draws are all zero takes no noise, and the rows that do take it put it on one
    square -- which is what such a Dirichlet draw looks like.

    Computed on the host in float64; device: where the int32 tensor goes (None: the
    host)."""
    alpha = float(alpha)
    if not ALPHA_MIN <= alpha <= ALPHA_MAX:  # (a nan fails both comparisons)
        raise ValueError("alpha must be in [%g, %g]" % (ALPHA_MIN, ALPHA_MAX))
    n = L.OTH_NOISE_TABLE
    p = (torch.arange(n, dtype=torch.float64) + 0.5) / float(n)
    q = gamma_quantiles(alpha, p)
    table = torch.round(q / q[-1] * float(L.OTH_NOISE_G_MAX - 1)).to(torch.int32)
    return table if device is None else table.to(device)


class RootNoise(object):
    """Root noise as AlphaZero-style self-play uses it: the root's priors become
    (1 - epsilon) p + epsilon eta, eta a Dirichlet(alpha) draw over the legal squares.
    `epsilon` is kept as round(256 epsilon), the unit of oth_puct_noise, and `table` is
    dirichlet_table(alpha); table_on(device) is its copy on a device, made once."""

    def __init__(self, epsilon=0.25, alpha=0.3):
        eps = int(round(256.0 * float(epsilon)))
        if not 0 <= eps <= 256:
            raise ValueError("epsilon must be in [0, 1]")
        self.epsilon, self.alpha = eps, float(alpha)
        self.table = dirichlet_table(alpha)
        self._on = {}

    def table_on(self, device):
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = self.table.to(device)
        return self._on[device]

    def __repr__(self):
        return "RootNoise(epsilon=%d/256, alpha=%g)" % (self.epsilon, self.alpha)
