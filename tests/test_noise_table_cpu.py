"""dirichlet_table (the gamma table of oth_puct_noise, made on the host in float64)
against its definition, and the statistics of the reference's draws at fixed seeds:
they are deterministic, so each bound either holds or does not.

The bounds: chi-square at p = 1e-6 (15 degrees of freedom: 52.0); a sample correlation
of R independent pairs has standard deviation 1 / sqrt(R), so 6 / sqrt(R) is six of
them; a two-sample Kolmogorov-Smirnov distance of two samples of n from one
distribution exceeds c sqrt(2 / n) with probability 2 exp(-2 c^2), which is 1e-6 at
c = 2.69."""
import math

import numpy as np
import pytest
import torch

import noise_ref as nf
import rng_ref as rng

ALPHAS = (0.03, 0.3, 1.0, 10.0)
TOP = (1 << 24) - 1
CHI2_DF15_P1E6 = 52.0  # the upper 1e-6 quantile of chi-square with 15 degrees of freedom (51.996)


def table(alpha):
    from gymothelloenv_amd.noise import dirichlet_table
    return dirichlet_table(alpha)


def P(alpha, x):
    """The regularised lower incomplete gamma function at x >= 0, float64."""
    x = torch.clamp(torch.as_tensor(x, dtype=torch.float64), min=0.0)
    return torch.special.gammainc(torch.full_like(x, float(alpha)), x)


@pytest.mark.parametrize("alpha", ALPHAS)
def test_the_table_is_its_definition(alpha):
    from gymothelloenv_amd.noise import gamma_quantiles
    t = table(alpha)
    assert t.dtype == torch.int32 and t.shape == (4096,) and t.device.type == "cpu"
    tt = t.to(torch.int64)
    assert bool((tt[1:] >= tt[:-1]).all()) and int(tt[-1]) == TOP and int(tt[0]) >= 0
    p = (torch.arange(4096, dtype=torch.float64) + 0.5) / 4096.0
    q_top = float(gamma_quantiles(alpha, p[-1:])[0])
    assert abs(float(P(alpha, q_top)) - float(p[-1])) < 1e-12
    s = q_top / TOP
    # the rounding bound itself: entry t is q / s rounded, so the quantile lies within a step of t s
    lo, hi = P(alpha, (tt - 1).to(torch.float64) * s), P(alpha, (tt + 1).to(torch.float64) * s)
    assert bool((lo <= p + 1e-9).all()), float((lo - p).max())
    assert bool((p <= hi + 1e-9).all()), float((p - hi).max())


def test_small_alpha_is_mostly_zero():
    """An entry is zero where the quantile is below half a step s = q_4095 / (2^24 - 1), that is for the
    fraction P(alpha, s / 2) of the entries: x^alpha / Gamma(alpha + 1) next to zero, with s / 2 about 5e-8 more
    than half of them at alpha = 0.03 (e^(-0.03 * 16.8) = 0.60) and one in a hundred at alpha = 0.3."""
    from gymothelloenv_amd.noise import gamma_quantiles
    zeros = {}
    for a in (0.01, 0.03, 0.3, 10.0):
        s = float(gamma_quantiles(a, torch.tensor([4095.5 / 4096.0], dtype=torch.float64))[0]) / TOP
        zeros[a] = int((table(a) == 0).sum())
        assert abs(zeros[a] - 4096.0 * float(P(a, 0.5 * s))) <= 1.0, (a, zeros[a])
    assert zeros[0.01] > zeros[0.03] > 2048 > 410 > zeros[0.3] > 0 and zeros[10.0] == 0


def test_alpha_range():
    from gymothelloenv_amd.noise import dirichlet_table
    for bad in (0.0, 0.00999, 100.01, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            dirichlet_table(bad)
    for ok in (0.01, 100.0):
        assert int(dirichlet_table(ok)[-1]) == TOP


@pytest.mark.parametrize("alpha", ALPHAS)
def test_quantiles_against_scipy(alpha):
    stats = pytest.importorskip("scipy.stats")
    p = (np.arange(4096) + 0.5) / 4096.0
    q = stats.gamma.ppf(p, alpha)
    want = np.round(q / q[-1] * TOP)
    assert np.abs(table(alpha).numpy().astype(np.int64) - want.astype(np.int64)).max() <= 1


# ------------------------------------------------------------------ the draws
SEED, COUNTER = 0x0123456789ABCDEF, 2 ** 40 + 17


def test_table_index_is_uniform():
    u = nf.words(8, 1024, SEED, 0, 0, COUNTER)  # 1,024 boards x 64 squares
    assert u.size == 65536
    assert rng.chi2_uniform((u >> np.uint32(28)).astype(np.int64).ravel(), 16) < CHI2_DF15_P1E6
    # ... and at another counter and key, on two-word boards
    u = nf.words(16, 256, SEED ^ (1 << 63), 5, 2 ** 32 - 3, COUNTER + 1)
    assert u.size == 65536
    assert rng.chi2_uniform((u >> np.uint32(28)).astype(np.int64).ravel(), 16) < CHI2_DF15_P1E6


def corr(x, y):
    x, y = x.astype(np.float64).ravel(), y.astype(np.float64).ravel()
    return float(np.corrcoef(x, y)[0, 1]), x.size


@pytest.mark.parametrize("alpha", (0.3, 1.0))
def test_draws_are_uncorrelated(alpha):
    t = table(alpha).numpy().astype(np.int64)
    g = t[nf.words(8, 1024, SEED, 0, 0, COUNTER) >> np.uint32(20)]
    for what, (r, R) in (("adjacent squares", corr(g[:, :-1], g[:, 1:])),
                         ("squares of one Philox block", corr(g[:, 0::4], g[:, 1::4])),
                         ("adjacent blocks", corr(g[:, 3:-1:4], g[:, 4::4])),
                         ("adjacent env ids", corr(g[:-1], g[1:]))):
        assert abs(r) < 6.0 / math.sqrt(R), (what, r, R)
    g2 = t[nf.words(8, 1024, SEED, 0, 0, COUNTER + 1) >> np.uint32(20)]
    r, R = corr(g, g2)
    assert abs(r) < 6.0 / math.sqrt(R), ("adjacent counters", r, R)


def ks_two_sample(x, y):
    x, y = np.sort(x), np.sort(y)
    both = np.concatenate([x, y])
    return float(np.abs(np.searchsorted(x, both, side="right") / x.size -
                        np.searchsorted(y, both, side="right") / y.size).max())


def test_eta_is_a_dirichlet_draw():
    k, alpha, n = 4, 0.3, 16384
    eta = nf.eta_rows(k, table(alpha).numpy(), SEED, COUNTER, n)
    assert eta.shape == (n, k) and np.abs(eta.sum(1) - 1.0).max() < 1e-4
    want = np.random.default_rng(20240229).dirichlet([alpha] * k, n)
    bound = 2.69 * math.sqrt(2.0 / n)
    assert abs(bound - 0.0297) < 5e-5
    for j in range(k):  # the issue's check is component 0; the others hold the same bound
        D = ks_two_sample(eta[:, j], want[:, j])
        assert D < bound, (j, D)
