"""oracle/weights_exact.py against brute force: ``fractions.Fraction`` on tiny
inputs, ``math.fsum`` (correctly rounded sums of doubles), and the edges the
device tests lean on -- subnormals, 2^+-1000 scalings, zeros.  Host only."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import weights_exact as wx


def F(v):
    return Fraction(float(v))


def rnd(fr):
    """A Fraction rounded once to float64."""
    return wx.ratio(fr.numerator, fr.denominator)


def tiny_weights(rng, n, kind):
    if kind == "uniform":
        return rng.uniform(size=n)
    if kind == "decades":
        return 10.0 ** rng.uniform(-300, 0, n)
    if kind == "subnormal":
        return rng.integers(0, 1 << 20, n) * 5e-324
    if kind == "zeros":
        return np.where(rng.uniform(size=n) < 0.6, 0.0, rng.uniform(size=n))
    if kind == "big":
        return np.ldexp(rng.uniform(0.5, 1, n), 1000)
    raise ValueError(kind)


KINDS = ["uniform", "decades", "subnormal", "zeros", "big"]


def test_to_ints_is_exact():
    rng = np.random.default_rng(0)
    a = np.r_[tiny_weights(rng, 20, "decades"), 0.0, -0.0, 5e-324, -1.5e300,
              2.0 ** -1074, 2.0 ** 1023]
    m, e = wx.to_ints(a)
    for v, k in zip(a, m):
        assert Fraction(k) * Fraction(2) ** e == F(v)
    m, e = wx.to_ints(np.zeros(3))
    assert list(m) == [0, 0, 0]
    with pytest.raises(ValueError):
        wx.to_ints(np.array([1.0, np.inf]))


def test_ratio_rounds_once():
    # halfway cases of the subnormal grid, ties to even, overflow, 0 / 0
    assert wx.ratio(1, 1, -1075) == 0.0
    assert wx.ratio(3, 1, -1075) == 2 * 5e-324
    assert wx.ratio(3, 2, -1074) == 2 * 5e-324
    assert wx.ratio((1 << 53) + 1, 1, 0) == float(1 << 53)
    assert wx.ratio((1 << 53) + 3, 1, 0) == float((1 << 53) + 4)
    assert wx.ratio(1, 1, 1024) == math.inf
    assert wx.ratio(-1, 1, 1024) == -math.inf
    assert math.isnan(wx.ratio(0, 0))
    assert wx.ratio(1, 3) == 1 / 3


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 2, 17])
def test_exact_sums_vs_fractions(kind, n):
    rng = np.random.default_rng(n)
    w = tiny_weights(rng, n, kind)
    if not w.any():
        w[0] = 5e-324
    r = wx.exact_sums(w)
    S = sum(F(v) for v in w)
    S2 = sum(F(v) ** 2 for v in w)
    assert r.sum == rnd(S) and r.sum_sq == rnd(S2) and r.max == w.max()
    assert r.ess == rnd(S * S / S2)
    assert list(r.normalised) == [rnd(F(v) / S) for v in w]
    if math.isfinite(rnd(S)):
        assert r.sum == math.fsum(w)
    if kind == "uniform":        # squares of doubles are not doubles: a bound
        assert abs(r.sum_sq - math.fsum(w * w)) <= n * wx.EPS * r.sum_sq


@pytest.mark.parametrize("k", [-1000, -600, -520, 500, 520])
def test_exact_sums_are_scale_free(k):
    """2^k w is exact here, so the ESS and the normalised weights do not move
    -- where float64 (sum w)^2 / sum w^2 gives NaN, inf or garbage."""
    rng = np.random.default_rng(5)
    w = rng.uniform(0.5, 1.5, 300) * 1e-3      # 2^-1000 w stays normal
    base = wx.exact_sums(w)
    ws = np.ldexp(w, k)
    assert np.array_equal(np.ldexp(ws, -k), w)
    r = wx.exact_sums(ws)
    assert r.ess == base.ess and np.array_equal(r.normalised, base.normalised)
    assert r.sum == math.ldexp(base.sum, k)
    with np.errstate(all="ignore"):
        naive = ws.sum() ** 2 / (ws ** 2).sum()
    if abs(k) >= 520:
        assert not abs(naive - base.ess) <= 1e-9 * base.ess


def test_exact_sums_edges():
    r = wx.exact_sums(np.array([0.375]))
    assert r.ess == 1.0 and list(r.normalised) == [1.0]
    r = wx.exact_sums(np.full(256, 0.1))
    assert r.ess == 256.0 and (r.normalised == 1 / 256).all()
    r = wx.exact_sums(np.zeros(4))
    assert r.sum == 0.0 and math.isnan(r.ess) and np.isnan(r.normalised).all()
    r = wx.exact_sums(np.r_[1.0, np.full(1000, 1e-10)])
    assert r.ess == pytest.approx(1.0 + 2e-7, abs=1e-13)
    assert wx.exact_sums(np.r_[1.0, np.full(1000, 1e-30)]).ess == 1.0


@pytest.mark.parametrize("kind", KINDS)
def test_exact_prefix(kind):
    rng = np.random.default_rng(11)
    w = tiny_weights(rng, 40, kind)
    p = wx.exact_prefix(w)
    run = Fraction(0)
    for i, v in enumerate(w):
        run += F(v)
        assert Fraction(p.ints[i]) * Fraction(2) ** p.e == run
        assert p.values[i] == rnd(run)
        if math.isfinite(p.values[i]):
            assert p.values[i] == math.fsum(w[:i + 1])
    assert (np.diff(p.values) >= 0).all()
    assert p.values[0] == w[0]


def _moments_fraction(X, w):
    N, d = X.shape
    S = sum(F(v) for v in w)
    m = [sum(F(w[i]) * F(X[i, a]) for i in range(N)) / S for a in range(d)]
    cov = [[sum(F(w[i]) * (F(X[i, a]) - m[a]) * (F(X[i, b]) - m[b])
                for i in range(N)) / S for b in range(d)] for a in range(d)]
    return m, cov


@pytest.mark.parametrize("case", ["plain", "offset", "scales", "const", "zero_w", "n1"])
def test_exact_moments_vs_fractions(case):
    rng = np.random.default_rng(3)
    N, d = (1, 3) if case == "n1" else (9, 3)
    X = rng.standard_normal((N, d))
    w = rng.uniform(size=N)
    if case == "offset":
        X += 1e10
    elif case == "scales":
        X *= np.array([1e-100, 1.0, 1e100])
    elif case == "const":
        X[:, 1] = 0.1
    elif case == "zero_w":
        w[::2] = 0.0
    r = wx.exact_moments(X, w)
    m, cov = _moments_fraction(X, w)
    assert r.own_error == 0.0
    assert list(r.mean) == [rnd(v) for v in m]
    for a in range(d):
        for b in range(d):
            assert r.cov[a, b] == rnd(cov[a][b]), (a, b)
    assert r.sum == math.fsum(w) and r.max == w.max()
    if case == "const":
        assert r.cov[1, 1] == 0.0 and r.mean[1] == 0.1
    if case == "n1":
        assert not r.cov.any()
    Mref = [float(sum(F(w[i]) * abs(F(X[i, a])) for i in range(N)) / sum(map(F, w)))
            for a in range(d)]
    np.testing.assert_allclose(r.M, Mref, rtol=1e-14)
    Aref = float(sum(F(w[i]) * abs(F(X[i, 0]) - m[0]) * abs(F(X[i, 2]) - m[2])
                     for i in range(N)) / sum(map(F, w)))
    assert r.A[0, 2] == pytest.approx(Aref, rel=1e-6)   # |x - m| with m rounded


@pytest.mark.parametrize("offset,scale", [(0.0, 1.0), (1e6, 1.0), (1e10, 1.0),
                                          (0.0, 1e100), (3.0, 1e-100)])
def test_double_double_moments_within_their_stated_error(offset, scale):
    """The route for large N d^2 against the integer route, in the units its
    own_error is stated in."""
    rng = np.random.default_rng(8)
    N, d = 3001, 4
    X = (rng.standard_normal((N, d)) + offset) * scale
    X[:, 3] *= 1e-3
    w = rng.exponential(size=N)
    w[5] = 0.0
    ex = wx.exact_moments(X, w, force_exact=True)
    dd = wx._dd_moments(X, w)
    assert 0 < dd.own_error < 3e-16
    assert (np.abs(dd.mean - ex.mean) <= dd.own_error * ex.M).all()
    tol = dd.own_error * ex.A + dd.own_error ** 2 * np.outer(ex.M, ex.M)
    assert (np.abs(dd.cov - ex.cov) <= tol).all(), np.max(np.abs(dd.cov - ex.cov) / tol)
    # float64 two-pass numpy on the same input, for scale: far outside that
    c = X - (w @ X) / w.sum()
    npcov = (w[:, None] * c).T @ c / w.sum()
    if offset >= 1e6:
        assert (np.abs(npcov - ex.cov) > tol).any()


def test_importance_weight_exact():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    lp = np.array([0.0, -3.25, 100.0, -700.0, 10.0, -745.0, 709.0, 711.0])
    lt = np.array([0.0, 2.5, -200.0, 45.0, 10.0, 0.25, -0.5, 0.0])
    aw = np.linspace(0.5, 2.0, len(lp))
    for scale, acc in ((1.0, None), (0.3, None), (0.3, aw)):
        got = wx.importance_weight_exact(lp, lt, scale, acc)
        for i in range(len(lp)):
            v = mp.exp(mp.mpf(float(lp[i])) - mp.mpf(float(lt[i]))) * mp.mpf(scale)
            if acc is not None:
                v *= mp.mpf(float(acc[i]))
            if v > mp.mpf(1.7976931348623157e308):
                assert got[i] == math.inf
            elif v >= mp.mpf(2.2250738585072014e-308):
                assert abs(mp.mpf(float(got[i])) - v) <= v * mp.mpf(2) ** -53
            else:     # subnormal: half a spacing
                assert abs(mp.mpf(float(got[i])) - v) <= mp.mpf(2) ** -1075
    assert wx.importance_weight_exact([0.0], [0.0], 0.3)[0] == 0.3
    assert wx.importance_weight_exact([1.0], [1.0], 1.0, [0.7])[0] == 0.7
    # IEEE specials
    inf, nan = math.inf, math.nan
    g = wx.importance_weight_exact([-inf, 0.0, nan, 0.0, -inf, 0.0],
                                   [0.0, -inf, 0.0, nan, -inf, 0.0], 0.3,
                                   [1.0, 1.0, 1.0, 1.0, 1.0, nan])
    assert g[0] == 0.0 and g[1] == inf and np.isnan(g[2:]).all()
