"""The stochastic-acceptance kernels (pyabc_amd/csrc/abc_stochastic.hip and
importance_weights_kernel of abc_reduce.hip) against references of higher
precision than float64, at the sizes where their code paths change.

References, all computed on the host from the same float64 inputs:
  * per-row kernel values: mpmath at 50 digits (ref_cont / ref_count);
  * the long reductions of abc_temper_sums and abc_importance_weights:
    np.longdouble terms, numpy's pairwise sum (ref_temper / ref_iw);
  * abc_stochastic_accept and the host drivers: the oracle.stochastic replay,
    which is their specification.
The CPU tests at the top hold the helpers themselves to scipy / the oracle
on the golden inputs (1e-12), so the references are tested without a GPU.

Tolerances: 1e-12 relative for kernel values and the temperature sums (all
terms positive, exp of an argument bounded by 100 carries at most
100 * 2^-53 relative error, the blocked sum a few ulps), 1e-13 for the
importance and acceptance weights, masks and maxima exact.  The count
kernels are measured in units of 2^-53 * sum |term| (see
test_kernel_count_scales).
"""
import functools
import math
import types

import mpmath
import numpy as np
import pytest
from scipy import stats

import oracle.stochastic as ost

gpu_mark = pytest.mark.gpu

LD = np.longdouble
MP = mpmath.mp.clone()
MP.dps = 50
INF = np.inf
U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def dev():
    from pyabc_amd import gpu
    return gpu.require_device()


def T(a, dtype=None):
    from pyabc_amd import gpu
    return gpu.as_dev(a, dtype=dtype)


def I32(a):
    import torch
    return T(np.asarray(a, dtype=np.int32), dtype=torch.int32)


def host(t):
    return t.cpu().numpy()


def same_specials(got, ref):
    """NaN and +-inf sit at the same places; returns the finite mask."""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf)
    assert np.array_equal(got[inf], ref[inf])
    return np.isfinite(ref)


def close(got, ref, rtol):
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    fin = same_specials(got, ref)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=rtol, atol=0)


# ---- references ---------------------------------------------------------------

def ref_temper(dens, lr, lr_sub, pdf_norm, scale_log, mode, beta, shift):
    """The formulas above temper_partial_kernel in longdouble -> (a, b).
    A NaN density has acceptance probability 0 in modes 0 and 3."""
    lr = np.asarray(lr, dtype=np.float64)
    if mode == 2:
        li = lr if lr_sub is None else lr - np.asarray(lr_sub, np.float64)
        return float(np.max(li)) if li.size else -INF, 0.0
    with np.errstate(all="ignore"):
        d = np.asarray(dens, dtype=np.float64).astype(LD)
        l = d - LD(pdf_norm) if scale_log else np.log(d / LD(pdf_norm))
        bl = np.zeros_like(l) if beta == 0.0 else LD(beta) * l
        if mode == 1:
            t = lr.astype(LD) * np.exp(bl)
            return float(np.sum(t)), float(np.sum(t * t))
        pacc = np.exp(np.minimum(bl, LD(0)))
        pacc[np.isnan(l)] = 0
        if mode == 3:
            w = lr.astype(LD)
        else:
            li = lr.astype(LD)
            if lr_sub is not None:
                li = li - np.asarray(lr_sub, np.float64).astype(LD)
            w = np.exp(li - LD(shift))
        return float(np.sum(w * pacc)), float(np.sum(w))


def ref_iw(lp, lt, scale, acc_w):
    with np.errstate(all="ignore"):
        v = np.exp(np.asarray(lp).astype(LD) - np.asarray(lt).astype(LD)) * LD(scale)
        if acc_w is not None:
            v = v * np.asarray(acc_w).astype(LD)
    return v.astype(np.float64)


def ref_cont(kind, x, cols, x0k, par, c, U=None):
    """Kinds 0-2 of abc_kernel_logpdf, exact for the float64 inputs (c and U
    as given) -> float64 [B], correctly rounded."""
    f = MP.mpf
    x0 = [f(float(v)) for v in x0k]
    cm = f(float(c))
    if kind == 2:
        K, r = U.shape
        Uc = [[f(float(U[j, q])) for j in range(K)] for q in range(r)]
    else:
        pm = [f(float(v)) for v in par]
    out = np.empty(x.shape[0])
    for b in range(x.shape[0]):
        df = [f(float(x[b, cj])) - x0[j] for j, cj in enumerate(cols)]
        if kind == 0:
            v = -(cm + MP.fsum(d * d / p for d, p in zip(df, pm))) / 2
        elif kind == 1:
            v = -(cm + MP.fsum(abs(d) / p for d, p in zip(df, pm)))
        else:
            v = -(cm + MP.fsum(MP.fdot(df, u) ** 2 for u in Uc)) / 2
        out[b] = float(v)
    return out


NAN_, ZERO_ = "nan", "zero"


def _count_terms(kind, k, m):
    """The p-free part of one element: NAN_ / ZERO_ or (sum, sum |term|) of
    its lgamma / Poisson terms; k the observed count, m = trunc(x)."""
    f = MP.mpf
    if kind == 3:
        if not m >= 0:
            return NAN_
        if k < 0:
            return ZERO_
        if k == 0:
            a = f(0)
        elif m == 0:
            return ZERO_                       # k log 0
        else:
            a = f(k) * MP.log(f(m))
        t = [a, -MP.loggamma(f(k) + 1), -f(m)]
    elif kind == 4:
        if not m >= 0:
            return NAN_
        if k < 0 or k > m:
            return ZERO_
        t = [MP.loggamma(f(m) + 1), -MP.loggamma(f(k) + 1),
             -MP.loggamma(f(m) - f(k) + 1)]
    else:
        if not m > 0:
            return NAN_
        if k < 0:
            return ZERO_
        t = [MP.loggamma(f(m) + f(k)), -MP.loggamma(f(k) + 1),
             -MP.loggamma(f(m))]
    return MP.fsum(t), MP.fsum(abs(v) for v in t)


def _xlogy(a, logb):
    """a * log b with 0 * log 0 = 0; logb None stands for log 0 = -inf."""
    if a == 0:
        return MP.mpf(0)
    return None if logb is None else MP.mpf(a) * logb


def ref_count(kind, x, cols, x0k, ps):
    """Kinds 3-5 for every p of ps -> {p: (value float64 [B], exact [B] of
    mpf or None, mag float64 [B])}: value with NaN / -inf where the model
    has them, exact and mag = sum_j sum_terms |term| on the finite rows.
    p = 0 is outside scipy's negative binomial (NaN)."""
    f = MP.mpf
    B = x.shape[0]
    m = np.trunc(np.asarray(x, np.float64)[:, list(cols)])
    base = [[_count_terms(kind, float(x0k[j]), float(m[b, j]))
             for j in range(len(cols))] for b in range(B)]
    res = {}
    for p in ps:
        lp = None if p == 0 else MP.log(f(p))
        lq = None if p == 1 else MP.log(1 - f(p))
        val, exact, mag = np.empty(B), [None] * B, np.zeros(B)
        for b in range(B):
            s, a, state = f(0), f(0), None
            for j, e in enumerate(base[b]):
                if e == NAN_ or (kind == 5 and p == 0):
                    state = NAN_
                    break
                if e == ZERO_:
                    state = ZERO_
                    continue
                k, mm = float(x0k[j]), float(m[b, j])
                if kind == 3:
                    extra = []
                elif kind == 4:
                    extra = [_xlogy(k, lp), _xlogy(mm - k, lq)]
                else:
                    extra = [None if lp is None else f(mm) * lp, _xlogy(k, lq)]
                if any(v is None for v in extra):
                    state = ZERO_
                    continue
                s += e[0] + MP.fsum(extra)
                a += e[1] + MP.fsum(abs(v) for v in extra)
            if state is None:
                val[b], exact[b], mag[b] = float(s), s, float(a)
            else:
                val[b] = np.nan if state == NAN_ else -INF
        res[p] = (val, exact, mag)
    return res


def count_units(got, exact, mag):
    """e = |got - exact| / (2^-53 sum |term|) on the finite rows (0 where a
    row without terms is met exactly)."""
    e = np.zeros(len(exact))
    for b, ex in enumerate(exact):
        if ex is None:
            continue
        err = abs(MP.mpf(float(got[b])) - ex)
        if mag[b] == 0.0:
            e[b] = 0.0 if err == 0 else INF
        else:
            e[b] = float(err / (MP.mpf(U53) * MP.mpf(float(mag[b]))))
    return e


def scipy_count(kind, x, cols, x0k, p):
    xi = np.asarray(np.asarray(x)[:, list(cols)], dtype=int)
    ki = np.asarray(x0k, dtype=int)
    with np.errstate(all="ignore"):
        if kind == 3:
            return np.sum(stats.poisson.logpmf(k=ki, mu=xi), axis=1)
        if kind == 4:
            return np.sum(stats.binom.logpmf(k=ki, n=xi, p=p), axis=1)
        return np.sum(stats.nbinom.logpmf(k=ki, n=xi, p=p), axis=1)


KIND_NAME = {0: "independent_normal", 1: "independent_laplace", 2: "normal",
             3: "poisson", 4: "binomial", 5: "negative_binomial"}


# ---- inputs ---------------------------------------------------------------------

SHAPES = [(1, 1, 1), (255, 5, 5), (256, 7, 3), (257, 40, 40), (1000, 300, 17)]


def make_cols(S, K, rng):
    """A random permutation subset of range(S); reversed for (S, K) = (5, 5)."""
    if (S, K) == (5, 5):
        return np.arange(S)[::-1].copy()
    return rng.permutation(S)[:K]


def fill_unused(x, cols, rng, nan):
    unused = np.setdiff1d(np.arange(x.shape[1]), cols)
    x[:, unused] = np.nan if nan else rng.normal(0, 50, (x.shape[0], unused.size))


@functools.lru_cache(maxsize=None)
def cont_case(kind, shape, deficient=False):
    """(x, cols, x0k, par, c, U) of a continuous kind: parameters over
    1e-6 .. 1e6 (kinds 0, 1), an SPD covariance conditioned 1e6 whitened by
    psd_whitening (kind 2; two zero eigenvalues when deficient).  The rows
    are 0.1, 1, 3 and 1000 kernel widths off x_0, so that log values near 0
    and below -745 both occur.  The widest shape has NaN in unused columns."""
    from pyabc_amd.transition.multivariatenormal import psd_whitening
    B, S, K = shape
    rng = np.random.default_rng(1000 * kind + S + 7 * deficient)
    cols = make_cols(S, K, rng)
    x0k = rng.normal(0, 3, K)
    width = np.array([0.1, 1.0, 3.0, 1000.0])[np.arange(B) % 4][:, None]
    n = rng.standard_normal((B, K)) * width
    x = np.empty((B, S))
    U = None
    if kind == 2:
        Q = np.linalg.qr(rng.standard_normal((K, K)))[0]
        ev = 10.0 ** (np.linspace(-3, 3, K) if K > 1 else np.zeros(1))
        if deficient:
            ev[:2] = 0.0
        cov = (Q * ev) @ Q.T
        cov = 0.5 * (cov + cov.T)
        psd = psd_whitening(cov)
        assert psd["rank"] == K - 2 * deficient
        U = np.ascontiguousarray(psd["U"])
        c = psd["rank"] * math.log(2 * math.pi) + psd["log_pdet"]
        x[:, cols] = x0k + n @ psd["L"].T
        par = np.zeros(1)
    else:
        par = 10.0 ** rng.uniform(-6, 6, K)
        if kind == 0:
            c = float(np.sum(np.log(2) + np.log(np.pi) + np.log(par)))
            x[:, cols] = x0k + n * np.sqrt(par)
        else:
            c = float(np.sum(np.log(2) + np.log(par)))
            x[:, cols] = x0k + n * par
    fill_unused(x, cols, rng, nan=(S == 300))
    ref = ref_cont(kind, x, cols, x0k, par, c, U)
    return x, cols, x0k, par, c, U, ref


COUNT_P = (0.01, 0.25, 0.5, 0.75, 0.99)
COUNT_CASES = [((1, 1, 1), 1e3), ((255, 5, 5), 10.0), ((256, 7, 3), 1e3),
               ((257, 40, 40), 1e6), ((1000, 300, 17), 1e9),
               ((255, 5, 5), 1e9), ((256, 7, 3), 1e6)]


@functools.lru_cache(maxsize=None)
def count_case(kind, shape, scale):
    """Counts at one scale: observed k_j = scale * U(0.5, 1.5); simulated
    Poisson means around k, binomial n = k + scale * U(0, 2), negative
    binomial n = scale * U(0.5, 1.5); half of the rows carry a fractional
    part (truncated by the kernel).  -> inputs, the mpmath reference per p,
    scipy's value per p."""
    B, S, K = shape
    rng = np.random.default_rng(int(100 * kind + S + math.log10(scale)))
    cols = make_cols(S, K, rng)
    x0k = np.floor(scale * rng.uniform(0.5, 1.5, K))
    if kind == 3:
        m = np.floor(x0k * (1 + rng.normal(0, 0.1, (B, K)))) + 1
    elif kind == 4:
        m = x0k + np.floor(scale * rng.uniform(0, 2, (B, K)))
    else:
        m = np.floor(scale * rng.uniform(0.5, 1.5, (B, K))) + 1
    m[::2] += rng.uniform(0, 0.9, m[::2].shape)
    x = np.empty((B, S))
    x[:, cols] = m
    fill_unused(x, cols, rng, nan=(S == 300))
    ps = COUNT_P if kind != 3 else (0.0,)
    ref = ref_count(kind, x, cols, x0k, ps)
    sci = {p: scipy_count(kind, x, cols, x0k, p) for p in ps}
    return x, cols, x0k, ps, ref, sci


CORNER_V = [0.0, 5.0, 7.0, 7.9, -0.5, 12.0000001, -3.0, 1000.0, 4.0]
CORNER_K = [(0.0, 5.0), (7.0, 7.0), (0.0, 0.0), (12.0, 4.0)]
CORNER_P = (0.0, 1.0, 0.3)


@functools.lru_cache(maxsize=None)
def corner_case(kind, ki):
    """Every pair of CORNER_V in the two kernel columns (2, 0) of a 3-column
    matrix against the observed pair CORNER_K[ki]: k = 0, n = k, k > n,
    negative and zero x, mu = 0, fractional x (7.9 -> 7, -0.5 -> 0,
    12.0000001 -> 12), and rows that mix a bad with a zero-probability
    element, at p = 0, 1 and 0.3."""
    pairs = np.array([(a, b) for a in CORNER_V for b in CORNER_V])
    x = np.full((pairs.shape[0], 3), np.nan)
    cols = np.array([2, 0])
    x[:, cols] = pairs
    x0k = np.array(CORNER_K[ki])
    ps = CORNER_P if kind != 3 else (0.0,)
    return x, cols, x0k, ps, ref_count(kind, x, cols, x0k, ps)


# ---- CPU: the references themselves -----------------------------------------

def _golden():
    import os
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, "stochastic.npz"))


def test_ref_cont_matches_oracle_on_golden():
    from pyabc_amd.transition.multivariatenormal import psd_whitening
    G = _golden()
    x, x0, var = G["cont_x"], G["cont_x0"], G["var"]
    cols = np.arange(4)
    c0 = float(np.sum(np.log(2) + np.log(np.pi) + np.log(var)))
    close(ref_cont(0, x, cols, x0, var, c0),
          ost.kernel_values("independent_normal", x, x0, par=var), 1e-12)
    c1 = float(np.sum(np.log(2) + np.log(var)))
    close(ref_cont(1, x, cols, x0, var, c1),
          ost.kernel_values("independent_laplace", x, x0, par=var), 1e-12)
    psd = psd_whitening(G["cov"])
    c2 = psd["rank"] * math.log(2 * math.pi) + psd["log_pdet"]
    close(ref_cont(2, x, cols, x0, None, c2, psd["U"]),
          ost.kernel_values("normal", x, x0, cov=G["cov"]), 1e-12)
    # a cols map that is no identity reads the same values
    perm = np.array([2, 0, 3, 1])
    xp = np.empty_like(x)
    xp[:, perm] = x
    close(ref_cont(0, xp, perm, x0, var, c0), ref_cont(0, x, cols, x0, var, c0), 0)


@pytest.mark.parametrize("kind", [3, 4, 5])
def test_ref_count_matches_oracle_on_golden(kind):
    G = _golden()
    x, x0 = G["count_x"], G["count_x0"]
    p = {3: 0.0, 4: float(G["p_binom"]), 5: float(G["p_nbinom"])}[kind]
    val, exact, mag = ref_count(kind, x, np.arange(4), x0, (p,))[p]
    with np.errstate(all="ignore"):
        want = ost.kernel_values(KIND_NAME[kind], x, x0, par=p)
    assert np.isfinite(want).sum() > 10
    close(val, want, 1e-12)
    assert (mag[np.isfinite(want)] >= np.abs(want[np.isfinite(want)])).all()


@pytest.mark.parametrize("kind", [3, 4, 5])
def test_ref_count_corners_match_scipy(kind):
    """NaN / -inf / 0 at the corners exactly where scipy.stats has them."""
    seen = set()
    for ki in range(len(CORNER_K)):
        x, cols, x0k, ps, ref = corner_case(kind, ki)
        for p in ps:
            val = ref[p][0]
            want = scipy_count(kind, x, cols, x0k, p)
            close(val, want, 1e-12)
            seen |= {"nan"} if np.isnan(val).any() else set()
            seen |= {"-inf"} if np.isneginf(val).any() else set()
            seen |= {"0"} if (val == 0).any() else set()
            seen |= {"fin"} if (np.isfinite(val) & (val != 0)).any() else set()
    assert seen == {"nan", "-inf", "0", "fin"}


@pytest.mark.parametrize("kind", [3, 4, 5])
def test_scipy_count_error_units(kind):
    """float64 scipy.stats stays within 2 units of 2^-53 * sum |term| on the
    inputs of test_kernel_count_scales: the anchor of the device's bound."""
    worst = 0.0
    for shape, scale in COUNT_CASES[:4]:
        x, cols, x0k, ps, ref, sci = count_case(kind, shape, scale)
        for p in ps:
            val, exact, mag = ref[p]
            assert np.isfinite(val).all()
            worst = max(worst, count_units(sci[p], exact, mag).max())
    print(f"kind {kind}: scipy max e = {worst:.3f}")
    assert worst <= 2.0


def test_ref_temper_matches_float64_objectives():
    G = _golden()
    pds, w = G["mar_pds"], G["mar_w"]
    for beta in (1.0, 0.37):
        a, b = ref_temper(pds, np.log(w), None, pds.max(), True, 0, beta, 0.0)
        want = np.sum(w * np.minimum(np.exp((pds - pds.max()) * beta), 1.0)) / np.sum(w)
        np.testing.assert_allclose(a / b, want, rtol=1e-12)
        a3, b3 = ref_temper(np.exp(pds), w, None, np.exp(pds.max()), False, 3, beta, 0.0)
        np.testing.assert_allclose(a3 / b3, want, rtol=1e-12)
        ep, ew = G["ess_pds"], G["ess_w"]
        s1, s2 = ref_temper(ep, ew, None, ep.max(), True, 1, beta, 0.0)
        v = ew * np.exp(ep - ep.max()) ** beta
        np.testing.assert_allclose(s1 * s1 / s2, np.sum(v) ** 2 / np.sum(v ** 2),
                                   rtol=1e-12)
    assert ref_temper(None, [1.0, 3.0, 2.0], [0.5, 4.0, 0.0], 0, True, 2, 0, 0)[0] == 2.0
    # a NaN density: weight in b only
    a, b = ref_temper([np.nan, 0.0], [0.0, 0.0], None, 0.0, True, 0, 1.0, 0.0)
    assert (a, b) == (1.0, 2.0)


# ---- 1. abc_temper_sums ---------------------------------------------------------

GRID = 256 * 1024
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, GRID, GRID + 1, 600001]
BETAS = (1.0, 0.37, 1e-3)


def temper_inputs(R, scale_log):
    rng = np.random.default_rng(R + (0 if scale_log else 17))
    dens = rng.normal(-4, 2, R)
    lr = np.clip(rng.normal(0, 1.5, R), -40, 40)
    sub = np.clip(rng.normal(0, 1.5, R), -40, 40)
    if scale_log:
        dens = np.clip(dens, -90, 90)
        pdf_norm = -3.0                # about a third of the records above it
    else:
        dens = np.exp(np.clip(dens, -90, 90))
        pdf_norm = float(dens.max())
    return dens, lr, sub, pdf_norm


def _check_sums(got, want, what):
    for g, w_, name in zip(got, want, "ab"):
        assert w_ > 0 and np.isfinite(w_), what
        assert abs(g - w_) <= 1e-12 * w_, (what, name, g, w_, (g - w_) / w_)


def _temper_sweep(R, scale_log):
    from pyabc_amd import gpu
    dens, lr, sub, pdf_norm = temper_inputs(R, scale_log)
    w = np.exp(lr)                       # linear weights of modes 1 and 3
    d_dens, d_lr, d_sub, d_w = T(dens), T(lr), T(sub), T(w)
    for use_sub in (False, True):
        hs, ds = (sub, d_sub) if use_sub else (None, None)
        want_max = ref_temper(None, lr, hs, 0.0, True, 2, 0.0, 0.0)[0]
        top = gpu.temper_sums(None, d_lr, 0.0, scale_log, gpu.TEMPER_MAX,
                              lr_sub=ds)[0]
        assert top == want_max
        for shift in (top, -3.25):
            for beta in BETAS:
                got = gpu.temper_sums(d_dens, d_lr, pdf_norm, scale_log, 0,
                                      beta, shift, lr_sub=ds)
                _check_sums(got, ref_temper(dens, lr, hs, pdf_norm, scale_log,
                                            0, beta, shift),
                            (R, 0, use_sub, shift, beta))
                for mode in (1, 3):      # linear weights: lr_sub / shift unused
                    got = gpu.temper_sums(d_dens, d_w, pdf_norm, scale_log,
                                          mode, beta, shift, lr_sub=ds)
                    _check_sums(got, ref_temper(dens, w, None, pdf_norm,
                                                scale_log, mode, beta, 0.0),
                                (R, mode, use_sub, shift, beta))


@gpu_mark
@pytest.mark.parametrize("R", SIZES)
def test_temper_sums_log_scale(dev, R):
    """Modes 0, 1, 3 (and the mode-2 shift) against longdouble at wave and
    block edges, one full grid (262 144), the first stride step (262 145)
    and two to three ragged stride passes through all 1024 partials."""
    _temper_sweep(R, True)


@gpu_mark
@pytest.mark.parametrize("R", [257, GRID + 1])
def test_temper_sums_lin_scale(dev, R):
    _temper_sweep(R, False)


@gpu_mark
@pytest.mark.parametrize("R", SIZES)
def test_temper_max_positions(dev, R):
    """Mode 2 is exact, wherever the maximum sits: first and last record and
    the first strided element (index 262 144)."""
    from pyabc_amd import gpu
    _, lr, sub, _ = temper_inputs(R, True)
    d_sub = T(sub)
    for pos in sorted({0, R - 1} | ({GRID} if R > GRID else set())):
        for hs, ds in ((None, None), (sub, d_sub)):
            v = lr.copy()
            v[pos] = 50.0 + (0.0 if hs is None else hs[pos])
            want = float(np.max(v if hs is None else v - hs))
            assert want >= 49.0
            got = gpu.temper_sums(None, T(v), 0.0, True, gpu.TEMPER_MAX,
                                  lr_sub=ds)[0]
            assert got == want, (R, pos)
    allneg = T(np.full(R, -INF))
    assert gpu.temper_sums(None, allneg, 0.0, True, gpu.TEMPER_MAX)[0] == -INF
    assert gpu.temper_sums(None, allneg, 0.0, True, gpu.TEMPER_MAX,
                           lr_sub=d_sub)[0] == -INF


@gpu_mark
def test_max_distance_device_population(dev):
    from pyabc_amd.acceptor import _max_distance, pdf_norm_max_found
    d = np.random.default_rng(3).normal(-4, 2, 300001)
    d[GRID + 5] = 9.5
    pop = types.SimpleNamespace(device_distance=T(d))
    assert _max_distance(pop) == d.max() == 9.5
    assert pdf_norm_max_found(prev_pdf_norm=3.0,
                              get_weighted_distances=lambda: pop) == 9.5
    assert pdf_norm_max_found(prev_pdf_norm=11.0,
                              get_weighted_distances=lambda: pop) == 11.0


R_EDGE = 257      # the second block has one live thread


@gpu_mark
def test_temper_beta_zero_keeps_weight(dev):
    """values ** 0 == 1 where the base is 0: at beta == 0 a -inf log density
    or a 0 lin density contributes its weight w_i to the ESS sums."""
    from pyabc_amd import gpu
    for scale_log in (True, False):
        dens, lr, _, pdf_norm = temper_inputs(R_EDGE, scale_log)
        w = np.exp(lr)
        dens[[0, 100, 256]] = -INF if scale_log else 0.0
        got = gpu.temper_sums(T(dens), T(w), pdf_norm, scale_log, 1, 0.0)
        want = (float(np.sum(w.astype(LD))), float(np.sum(w.astype(LD) ** 2)))
        assert np.isfinite(got).all()
        _check_sums(got, want, scale_log)
        _check_sums(got, ref_temper(dens, w, None, pdf_norm, scale_log, 1, 0.0, 0.0),
                    scale_log)


@gpu_mark
def test_temper_minus_inf_weight_and_clipping(dev):
    """lr = -inf records add 0 to both sums; densities above pdf_norm count
    with probability 1 in modes 0 and 3 and unclipped in mode 1."""
    from pyabc_amd import gpu
    dens, lr, sub, pdf_norm = temper_inputs(R_EDGE, True)
    lr[[0, 64, 256]] = -INF
    for hs in (None, sub):
        got = gpu.temper_sums(T(dens), T(lr), pdf_norm, True, 0, 0.37, -3.25,
                              lr_sub=None if hs is None else T(hs))
        keep = np.isfinite(lr)
        _check_sums(got, ref_temper(dens[keep], lr[keep], None if hs is None
                                    else hs[keep], pdf_norm, True, 0, 0.37, -3.25),
                    "minus inf")
    dens, lr, _, pdf_norm = temper_inputs(R_EDGE, True)
    dens += 5.0                          # most records above pdf_norm
    assert (dens > pdf_norm).sum() > 200
    w = np.exp(lr)
    ld = dens.astype(LD) - LD(pdf_norm)
    p1 = np.where(ld > 0, LD(1), np.exp(ld))
    for mode, wt in ((0, np.exp(lr.astype(LD))), (3, w.astype(LD))):
        got = gpu.temper_sums(T(dens), T(lr if mode == 0 else w), pdf_norm,
                              True, mode, 1.0, 0.0)
        _check_sums(got, (float(np.sum(wt * p1)), float(np.sum(wt))), mode)
        assert got[0] <= got[1]
    got = gpu.temper_sums(T(dens), T(w), pdf_norm, True, 1, 1.0)
    t = w.astype(LD) * np.exp(ld)
    _check_sums(got, (float(np.sum(t)), float(np.sum(t * t))), 1)
    assert got[0] > float(np.sum(w))


@gpu_mark
def test_temper_workspace_is_stateless(dev):
    """A call leaves nothing in the workspace that the next one reads: a
    1024-partial sum, then a max, then a two-block sum of another mode."""
    from pyabc_amd import gpu
    big = temper_inputs(600001, True)
    gpu.temper_sums(T(big[0]), T(big[1]), big[3], True, 0, 1.0, 0.0)
    dens, lr, sub, pdf_norm = temper_inputs(R_EDGE, True)
    w = np.exp(lr)
    assert gpu.temper_sums(None, T(lr), 0.0, True, 2)[0] == lr.max()
    got = gpu.temper_sums(T(dens), T(w), pdf_norm, True, 1, 0.37)
    _check_sums(got, ref_temper(dens, w, None, pdf_norm, True, 1, 0.37, 0.0), 1)
    got = gpu.temper_sums(T(dens), T(lr), pdf_norm, True, 0, 0.37, 0.5, lr_sub=T(sub))
    _check_sums(got, ref_temper(dens, lr, sub, pdf_norm, True, 0, 0.37, 0.5), 0)
    assert gpu.temper_sums(None, T(lr), 0.0, True, 2, lr_sub=T(sub))[0] == (lr - sub).max()


@gpu_mark
@pytest.mark.parametrize("scale_log", [True, False])
def test_temper_nan_density_records(dev, scale_log):
    """A record with a NaN density (a count kernel on a negative simulated
    count) is always rejected by the acceptor, so in modes 0 and 3 it adds
    its weight to b and nothing to a -- not probability 1, as
    exp(fmin(NaN, 0)) alone would make it.  Mode 1 is unchanged."""
    from pyabc_amd import gpu
    dens, lr, sub, pdf_norm = temper_inputs(R_EDGE, scale_log)
    w = np.exp(lr)
    bad = [0, 130, 256]
    dens[bad] = np.nan
    ok = np.ones(R_EDGE, bool)
    ok[bad] = False
    for beta in (1.0, 0.37, 0.0):
        got = gpu.temper_sums(T(dens), T(lr), pdf_norm, scale_log, 0, beta,
                              -3.25, lr_sub=T(sub))
        want = ref_temper(dens, lr, sub, pdf_norm, scale_log, 0, beta, -3.25)
        part = ref_temper(dens[ok], lr[ok], sub[ok], pdf_norm, scale_log, 0,
                          beta, -3.25)
        assert abs(want[0] - part[0]) <= 1e-15 * want[0] and want[1] > part[1]
        _check_sums(got, want, (0, beta))
        got = gpu.temper_sums(T(dens), T(w), pdf_norm, scale_log, 3, beta)
        _check_sums(got, ref_temper(dens, w, None, pdf_norm, scale_log, 3, beta, 0.0),
                    (3, beta))


# ---- 2. abc_kernel_logpdf ---------------------------------------------------------

def _logpdf(kind, x, cols, x0k, par, c, U=None, ret_lin=False):
    from pyabc_amd import gpu
    return host(gpu.kernel_logpdf(
        T(x), I32(cols), T(x0k), KIND_NAME[kind], T(np.atleast_1d(par)), c,
        U=None if U is None else T(U), ret_lin=ret_lin))


def _check_cont(kind, shape, deficient=False):
    x, cols, x0k, par, c, U, ref = cont_case(kind, shape, deficient)
    assert np.isfinite(ref).all()
    got = _logpdf(kind, x, cols, x0k, par, c, U)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
    lin = _logpdf(kind, x, cols, x0k, par, c, U, ret_lin=True)
    mid, gone = (ref >= -600) & (ref <= 0), ref < -745
    np.testing.assert_allclose(lin[mid], np.exp(ref[mid].astype(LD)).astype(float),
                               rtol=1e-10, atol=0)
    assert (lin[gone] == 0.0).all()
    return mid.sum(), gone.sum()


@gpu_mark
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("kind", [0, 1])
def test_kernel_independent(dev, kind, shape):
    """IndependentNormal / IndependentLaplace with parameters over 1e-6 ..
    1e6, through a cols map that is a permutation subset (reversed for
    S = K = 5; unused columns NaN for S = 300), log and lin scale."""
    mid, gone = _check_cont(kind, shape)
    if shape[0] > 1:
        assert mid > 0 and gone > 0


@gpu_mark
@pytest.mark.parametrize("shape", [(256, 7, 3), (1000, 300, 17), (257, 40, 40)],
                         ids=str)
def test_kernel_normal_full_rank(dev, shape):
    """NormalKernel factors of K = 3, 17, 40 (cov conditioned 1e6)."""
    mid, gone = _check_cont(2, shape)
    assert mid > 0 and gone > 0


@gpu_mark
def test_kernel_normal_rank_deficient(dev):
    """r = K - 2 < K (U is [K x r]), which the header allows and only the C
    ABI wrapper can pass: NormalKernel refuses a singular covariance."""
    x, cols, x0k, par, c, U, ref = cont_case(2, (255, 5, 5), True)
    assert U.shape == (5, 3)
    _check_cont(2, (255, 5, 5), True)


@gpu_mark
@pytest.mark.parametrize("case", COUNT_CASES, ids=str)
@pytest.mark.parametrize("kind", [3, 4, 5])
def test_kernel_count_scales(dev, kind, case):
    """Poisson / binomial / negative binomial at counts of 10 .. 1e9, where
    the lgamma terms cancel to a result many digits smaller than they are.
    The error is measured in units of the rounding of the terms,
        e = |got - exact| / (2^-53 * sum_j sum_terms |term|),
    and the device may take max(16, 8 x scipy's own maximum on the same
    inputs), scipy's being asserted <= 2 first.

    Measured maxima of e over these cases (Poisson / binomial / negative
    binomial): scipy on the CPU 0.55 / 1.15 / 1.24, the device on an MI355X
    0.61 / 1.19 / 1.18."""
    shape, scale = case
    x, cols, x0k, ps, ref, sci = count_case(kind, shape, scale)
    for p in ps:
        val, exact, mag = ref[p]
        assert np.isfinite(val).all()
        e_sci = count_units(sci[p], exact, mag).max()
        assert e_sci <= 2.0
        got = _logpdf(kind, x, cols, x0k, p, 0.0)
        same_specials(got, val)
        e_dev = count_units(got, exact, mag).max()
        print(f"kind {kind} {shape} scale {scale:g} p {p}: "
              f"scipy e = {e_sci:.3f}, device e = {e_dev:.3f}")
        assert e_dev <= max(16.0, 8.0 * e_sci)


@gpu_mark
@pytest.mark.parametrize("ki", range(len(CORNER_K)))
@pytest.mark.parametrize("kind", [3, 4, 5])
def test_kernel_count_corners(dev, kind, ki):
    """p = 0 / p = 1 / k = 0 / n = k / k > n (-inf) / negative x (NaN) /
    x = 0 for the negative binomial (NaN) / mu = 0 / fractional x truncated
    toward zero / NaN winning over -inf in one row: NaN and +-inf exactly
    where the reference has them (test_ref_count_corners_match_scipy holds
    the reference to scipy there), finite rows within 16 units.
    Named case: the negative binomial at p = 0 is NaN as in scipy (n > 0,
    0 < p <= 1); the kernel used to return -inf."""
    x, cols, x0k, ps, ref = corner_case(kind, ki)
    for p in ps:
        val, exact, mag = ref[p]
        got = _logpdf(kind, x, cols, x0k, p, 0.0)
        same_specials(got, val)
        assert count_units(got, exact, mag).max() <= 16.0
        lin = _logpdf(kind, x, cols, x0k, p, 0.0, ret_lin=True)
        assert np.array_equal(np.isnan(lin), np.isnan(val))
        assert (lin[np.isneginf(val)] == 0.0).all()
        assert (lin[val == 0.0] == 1.0).all()


# ---- 3. abc_stochastic_accept -------------------------------------------------------

ACC_B = [1, 255, 257, 5000]
ACC_IDX0 = [0, 2 ** 32 - 100, 2 ** 32 + 12345]
ACC_TEMPS = [1e-3, 1.0, 2.5, 1e6]
ACC_SEED, ACC_GEN = 20240607, 5


@functools.lru_cache(maxsize=None)
def accept_case(B, idx0, scale_log):
    """Densities with the corner rows in front (B >= 255), the replayed
    uniforms and, per (temperature, apply_iw), the oracle's (acc, mask, w)."""
    rng = np.random.default_rng(B + (0 if scale_log else 1))
    dens = rng.normal(-4, 2, B)
    c = -3.0
    if not scale_log:
        dens, c = np.exp(dens), math.exp(-3.0)
    if B >= 255:
        corner = ([np.nan, -INF, INF, 5.0, c] if scale_log else
                  [np.nan, 0.0, -0.25, INF, c, 2.0 * c])
        dens[:len(corner)] = corner
        dens[-1] = corner[1]             # an acc == 0 row in the last block
    u = ost.accept_uniform(ACC_SEED, ACC_GEN, idx0, B)
    out = {}
    for temp in ACC_TEMPS:
        with np.errstate(all="ignore"):
            acc = (np.exp((dens - c) * (1 / temp)) if scale_log
                   else (dens / c) ** (1 / temp))
        for iw in (True, False):
            mask, w = ost.stochastic_accept(dens, c, temp, scale_log, iw, u)
            out[temp, iw] = (acc, mask, w)
    return dens, c, u, out


def test_accept_reference_rows_off_the_boundary():
    """No reference row sits within 1e-9 of acc == u, so the device's mask
    has to be exact (seed chosen accordingly)."""
    gap = INF
    for B in ACC_B:
        for idx0 in ACC_IDX0:
            for log in (True, False):
                dens, c, u, out = accept_case(B, idx0, log)
                assert ((u >= 0) & (u < 1)).all()
                for temp in ACC_TEMPS:
                    acc = out[temp, True][0]
                    fin = np.isfinite(acc)
                    gap = min(gap, np.abs(u[fin] - acc[fin]).min())
    assert gap > 1e-9
    # the index really is 64-bit: streams 2^32 apart differ
    assert not np.array_equal(ost.accept_uniform(ACC_SEED, ACC_GEN, 0, 100),
                              ost.accept_uniform(ACC_SEED, ACC_GEN, 2 ** 32, 100))


@gpu_mark
@pytest.mark.parametrize("idx0", ACC_IDX0)
@pytest.mark.parametrize("B", ACC_B)
def test_stochastic_accept_grid(dev, B, idx0):
    """Mask exact, weights on all rows (1e-13, NaN positions equal), key =
    u - acc, over temperatures 1e-3 .. 1e6, both scales, both apply_iw, and
    candidate indices below, across and above 2^32."""
    from pyabc_amd import gpu
    for log in (True, False):
        dens, c, u, out = accept_case(B, idx0, log)
        d_dens = T(dens)
        for temp in ACC_TEMPS:
            for iw in (True, False):
                acc, mask, w = out[temp, iw]
                assert np.abs((u - acc)[np.isfinite(acc)]).min() > 1e-9
                key, accw = gpu.stochastic_accept(d_dens, c, temp, log, iw,
                                                  ACC_SEED, ACC_GEN, idx0)
                key, accw = host(key), host(accw)
                what = (B, idx0, log, temp, iw)
                assert np.array_equal(key <= 0, mask), what
                close(accw, w, 1e-13)
                assert (accw[acc == 0.0] == 0.0).all()
                with np.errstate(all="ignore"):
                    kref = u - acc
                fin = same_specials(key, kref)
                assert (np.abs(key[fin] - kref[fin])
                        <= 1e-13 * np.maximum(1.0, acc[fin])).all(), what
        if B >= 255:
            assert np.isnan(key[0]) and not mask[0]


# ---- 4. abc_importance_weights ------------------------------------------------------

@gpu_mark
@pytest.mark.parametrize("A", [1, 256, 257, 3001])
def test_importance_weights_scale_and_acc(dev, A):
    """prior / transition * scale * acceptance weight, the stochastic-acceptor
    path of the batched sampler, against longdouble (1e-13)."""
    from pyabc_amd import gpu
    rng = np.random.default_rng(A)
    lp = rng.normal(-5, 20, A)
    lt = lp - np.clip(rng.normal(0, 40, A), -100, 100)
    accw = rng.uniform(0, 3, A)
    accw[-1] = 2.75
    accw[0] = 0.0
    if A > 4:
        lp[1] = -INF
        lt[2] = -INF
        accw[1:3] = 1.5
    for scale in (1.0, 1 / 7):
        for aw in (None, accw):
            got = host(gpu.importance_weights(T(lp), T(lt), scale,
                                              None if aw is None else T(aw)))
            want = ref_iw(lp, lt, scale, aw)
            close(got, want, 1e-13)
            if A > 4:
                assert got[1] == 0.0 and got[2] == INF
            if aw is not None:
                assert got[0] == 0.0


# ---- 5. the host drivers at a realistic record count -------------------------------

R_HOST = 300001


@functools.lru_cache(maxsize=None)
def host_records():
    rng = np.random.default_rng(11)
    pds = rng.normal(-4, 2, R_HOST)
    lprev = rng.normal(-2, 1, R_HOST)
    lw = lprev + rng.normal(0, 1.5, R_HOST)
    return pds, lprev, lw


@functools.lru_cache(maxsize=None)
def host_population():
    """Densities and population weights whose ESS target (0.8 n) is met at
    an interior beta (T about 5.47), above the bound 1 / 7.5."""
    rng = np.random.default_rng(12)
    return host_records()[0], np.exp(rng.normal(0, 0.3, R_HOST))


@gpu_mark
def test_match_acceptance_rate_300k(dev):
    import pyabc_amd as pa
    from pyabc_amd.epsilon.temperature import match_acceptance_rate
    SL, SG = pa.distance.SCALE_LIN, pa.distance.SCALE_LOG
    pds, lprev, lw = host_records()
    w = np.exp(lw - lprev)
    d, dl, dp = T(pds), T(lw), T(lprev)
    c = float(np.quantile(pds, 0.999))
    got = match_acceptance_rate(d, dl, c, SG, 0.3, dp)
    want = ost.match_acceptance_rate(w, pds, c, True, 0.3)
    assert 1.0 < want < 1e3
    np.testing.assert_allclose(got, want, rtol=1e-9)
    lin = np.exp(pds)
    got = match_acceptance_rate(T(lin), T(w), math.exp(c), SL, 0.3, None,
                                log_form=False)
    np.testing.assert_allclose(got, ost.match_acceptance_rate(
        w, lin, math.exp(c), False, 0.3), rtol=1e-9)
    # obj(0) > 0: the rate at T = 1 already exceeds the target
    assert match_acceptance_rate(d, dl, pds.min(), SG, 0.3, dp) == 1.0
    assert ost.match_acceptance_rate(w, pds, pds.min(), True, 0.3) == 1.0
    # obj(-100) < 0: 80 % of the weight has density -inf, never accepted
    dead = pds.copy()
    dead[np.argsort(w)[-(R_HOST // 2):]] = -INF
    assert w[np.isneginf(dead)].sum() > 0.75 * w.sum()
    got = match_acceptance_rate(T(dead), dl, c, SG, 0.3, dp)
    with np.errstate(all="ignore"):
        want = ost.match_acceptance_rate(w, dead, c, True, 0.3)
    assert got == want == 1.0 / np.exp(-100)


@gpu_mark
@pytest.mark.parametrize("prev", [None, 7.5])
def test_ess_scheme_300k(dev, prev):
    import pyabc_amd as pa
    pds, w = host_population()
    pop = types.SimpleNamespace(device_distance=T(pds), device_w=T(w))
    got = pa.EssScheme()(t=1, get_weighted_distances=lambda: pop,
                         get_all_records=None, max_nr_populations=5,
                         pdf_norm=pds.max(), kernel_scale=pa.distance.SCALE_LOG,
                         prev_temperature=prev, acceptance_rate=0.3)
    want = ost.ess_temperature(pds, w, pds.max(), True, prev)
    assert 2.0 < want < 7.0
    np.testing.assert_allclose(np.ravel(got)[0], want, rtol=1e-5)
