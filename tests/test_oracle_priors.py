"""The oracle's replay of the t = 0 prior draw (oracle/sampler.py
propose_prior: the device's prior_draw1 / gamma_draw restated stream for
stream) draws from the distributions it claims to: every shape against
scipy's cdf.  tests/test_gpu_priors.py then holds the device to the replay
draw for draw, so together the device's draws are pinned to scipy."""
import numpy as np
from scipy import stats

import oracle.sampler as osamp

# (kind, device params [shape.., loc, scale] padded to 4): gamma below, at and
# above a = 1 (the a < 1 boost stream; a = 0.05 puts most mass next to 0),
# beta with either, both and neither shape below 1 (its second gamma stream,
# whose boost slot lies in the next coordinate's slot window), lognorm with a
# narrow and a wide s, laplace / expon / norm / uniform with loc and scale
SHAPES = [
    ("gamma", [0.05, 0.0, 1.0, 0.0]),
    ("gamma", [0.3, -1.0, 2.0, 0.0]),
    ("gamma", [1.0, 0.5, 0.25, 0.0]),
    ("gamma", [2.5, 0.0, 1.0, 0.0]),
    ("gamma", [50.0, 3.0, 0.1, 0.0]),
    ("beta", [0.5, 0.5, 0.0, 1.0]),
    ("beta", [0.7, 3.0, -2.0, 4.0]),
    ("beta", [1.0, 1.0, 1.0, 0.5]),
    ("beta", [2.0, 3.0, 0.0, 1.0]),
    ("beta", [30.0, 0.4, 0.0, 1.0]),
    ("lognorm", [0.1, 1.0, 2.0, 0.0]),
    ("lognorm", [2.0, -0.5, 0.3, 0.0]),
    ("laplace", [-1.5, 0.7, 0.0, 0.0]),
    ("expon", [2.0, 3.5, 0.0, 0.0]),
    ("norm", [1.0, 2.0, 0.0, 0.0]),
    ("uniform", [-1.0, 3.0, 0.0, 0.0]),
]
NSHAPE = {"norm": 0, "uniform": 0, "expon": 0, "laplace": 0, "lognorm": 1,
          "gamma": 1, "beta": 2}


def frozen(kind, p):
    """scipy's frozen distribution of a device (kind, params) pair."""
    n = NSHAPE[kind] + 2
    return getattr(stats, kind)(*[float(v) for v in p[:n]])


def test_prior_replay_draws_follow_scipy():
    """KS distance of n = 200 000 replayed draws per shape to scipy's cdf
    below 1.95 / sqrt(n) = 0.00436, the 0.1 % critical value of the
    Kolmogorov distribution (Q_KS(1.95) = 2 exp(-2 1.95^2) = 0.001); the
    seed is fixed, so the test is deterministic.  The shapes are the columns
    of one d = 16 draw, so coordinate k reads the slots 32 + 512 k + ..."""
    n = 200_000
    kinds = [k for k, _ in SHAPES]
    params = np.array([p for _, p in SHAPES])
    th, lp, att, margin = osamp.propose_prior(kinds, params, 9, 0, 1000, n, 10)
    assert (att == 1).all()
    assert margin.min() > 0.0 and np.isfinite(margin).all()
    bar = 1.95 / np.sqrt(n)
    worst = {}
    for k, (kind, p) in enumerate(SHAPES):
        ks = stats.kstest(th[:, k], frozen(kind, p).cdf).statistic
        worst[(kind, tuple(p))] = ks
        print(kind, p, "KS", ks)
    bad = {s: v for s, v in worst.items() if not v < bar}
    assert not bad, (bad, bar)
    # columns are independent streams: no two share draws (a slot collision
    # would make columns of the same family functionally dependent)
    u = np.column_stack([frozen(kind, p).cdf(th[:5000, k])
                         for k, (kind, p) in enumerate(SHAPES)])
    c = np.corrcoef(u, rowvar=False)
    np.fill_diagonal(c, 0.0)
    # |r| of 5000 independent pairs: sd 0.0141; 120 pairs, 5 sd
    assert np.abs(c).max() < 5 / np.sqrt(5000), np.abs(c).max()
    # the density of the accepted rows is scipy's at those rows
    ref = sum(frozen(kind, p).logpdf(th[:2000, k]) for k, (kind, p) in enumerate(SHAPES))
    np.testing.assert_allclose(lp[:2000], ref, rtol=1e-12)


def test_prior_replay_redraws_outside_support():
    """A lognorm with s = 200 under- or overflows exp(s n) for |n| > 3.5:
    those rows leave the support (the density is 0 at loc and at inf) and
    are re-drawn from the next attempt's slots; with max_attempts = 1 they
    give up (attempts = 2, logpdf -inf, theta the last draw).  The rows that
    stay have a finite logpdf, also next to either end of the doubles."""
    kinds, params = ["norm", "lognorm"], np.array([[0, 1, 0, 0], [200.0, 0.0, 1.0, 0]])
    th, lp, att, _ = osamp.propose_prior(kinds, params, 5, 0, 0, 100_000, 5)
    assert (att >= 1).all() and (att <= 2).all() and 5 <= (att == 2).sum() <= 120
    assert np.isfinite(lp).all() and (th[:, 1] > 0.0).all() and np.isfinite(th).all()
    th1, lp1, att1, _ = osamp.propose_prior(kinds, params, 5, 0, 0, 100_000, 1)
    out = att == 2
    np.testing.assert_array_equal(att1 == 2, out)
    assert np.isneginf(lp1[out]).all()
    assert (np.isinf(th1[out, 1]) | (th1[out, 1] == 0.0)).all()
    y = th[:, 1]
    assert (y < 1e-307).any() and (y > 1e305).any()   # draws at scipy's lossy ends
    ld = np.longdouble
    ly = np.log(y.astype(ld))
    exact = -(ly / 200) ** 2 / 2 - ly - np.log(200 * np.sqrt(2 * ld(np.pi)))
    l1 = osamp.prior_logpdf(th[:, 1:], ["lognorm"], params[1:])
    # terms up to 745 in size: 1e-12 is ten of their ulps
    np.testing.assert_allclose(l1, exact.astype(np.float64), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(th1[~out], th[~out])
    # the re-drawn rows come from attempt 1's slots: the same rows as a
    # one-attempt draw whose streams are shifted by 65536 slots
    r = osamp.prior_draws("norm", params[0], np.nonzero(out)[0], 65536 + 32, 0, 5)[0]
    np.testing.assert_array_equal(th[out, 0], r)
