"""The x3 density kernel over its limb-grid exponents, and the whole
MultivariateNormalTransition chain on shifted, scaled and ridge populations.

The kernel's error is set by the grid exponent E that x3_setup_kernel derives
from the population's largest whitened norm (abc_mvn_x3.hip): the dropped
class-3 limb products are bounded by 2^(2E-35) per coordinate whatever the
magnitude of the pair, so one far particle sets the error of every pair.  The
cases here put E where they want it -- a Gaussian bulk of 3000 with one
particle of weight 1e-9 placed at a chosen whitened norm -- and assert the
exponent and the route the transition reports (``x3_grid()``) before they
assert the density, at the project's contract: 1e-6 relative unhinted and
2e-6 hinted where mvn_x3_kernel answers, 2e-6 where the f64-MFMA kernel does,
for every candidate.  The cap between the two is read from the library
(``gpu.mvn_x3_max_exponent()``).

Reference: oracle/mvn_exact.py (direct differences, 40-digit whitening of the
reported covariance, longdouble log-sum-exp; exact integer sums for the fit).
tests/test_oracle_mvn_exact.py asserts the conditions on these inputs without
a GPU.
"""
import numpy as np
import pytest

from oracle import local_exact as le
from oracle import mvn_exact as me

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

X3_TOL, X3_TOL_HINTED, F64_TOL = 1e-6, 2e-6, 2e-6
RESCUE_RTOL = 1e-9       # fp64 rescue, in log density (test_mvn_x3_rescue_and_edges)
N_NEAR = 8               # candidates drawn around the outlier itself


@pytest.fixture(scope="module")
def dev():
    from pyabc_amd import gpu
    return gpu.require_device()


def _cols(d):
    return [f"p{k:02d}" for k in range(d)]


def _fit(X, w, scaling=1.0):
    import pyabc_amd as pa
    from pyabc_amd import gpu
    tr = pa.MultivariateNormalTransition(scaling=scaling)
    tr.fit_device(gpu.as_dev(X), gpu.as_dev(w), _cols(X.shape[1]))
    return tr


def _whitening(tr):
    """The device fit's own mean and whitening (full rank)."""
    tr.x3_grid()
    return tr._dev_mu.cpu().numpy(), tr._dev_U.cpu().numpy()


def _densities(tr, x, hint):
    from pyabc_amd import gpu
    xd = gpu.as_dev(x)
    hd = gpu.as_dev(hint, dtype=torch.int64)
    plain = tr.logpdf_device(xd).cpu().numpy()
    hinted = tr.logpdf_device(xd, hint=hd).cpu().numpy()
    return plain, hinted


def _rel(got, ref):
    return np.abs(np.expm1(got - ref))


def _bars(route):
    return (X3_TOL, X3_TOL_HINTED) if route == "x3" else (F64_TOL, F64_TOL)


def _proposals(tr, M, extra=None, extra_hint=None):
    """M proposals with their ancestors, plus extra rows (and their hints)."""
    th, _, anc, _ = tr.propose_device(M, seed=5, generation=1, idx0=0)
    x, hint = th.cpu().numpy(), anc.cpu().numpy().astype(np.int64)
    if extra is not None:
        x = np.vstack([x, extra])
        hint = np.concatenate([hint, np.asarray(extra_hint, dtype=np.int64)])
    return x, hint


def _around(tr, point, n, seed):
    """n points half a kernel width around ``point``."""
    rng = np.random.default_rng(seed)
    L = np.linalg.cholesky(np.atleast_2d(tr.cov))
    return point + 0.5 * rng.standard_normal((n, len(point))) @ L.T


_bulk = {}


def _bulk_whitening(d):
    """mu, U of the sweep population of dimension d without an outlier."""
    if d not in _bulk:
        X, w, _ = me.sweep_population(d)
        _bulk[d] = _whitening(_fit(X, w, me.SWEEP_SCALING[d]))
    return _bulk[d]


# ---- exponent sweep ------------------------------------------------------------

@pytest.mark.parametrize("d,label", me.sweep_cases())
def test_x3_exponent_sweep(dev, d, label):
    """d in {1, 2, 10, 25} x E = 5 (the bulk alone), 6, both edges of the
    E = 7 and E = 8 intervals and just past E = 8: the reported exponent is
    the one aimed at, the route is x3 up to the library's cap and f64 above
    it, and every candidate -- 400 proposals and 8 points around the outlier
    itself, whose pairs carry the largest limbs -- meets the contract,
    unhinted and hinted with its ancestor."""
    from pyabc_amd import gpu
    E_want, _ = me.SWEEP_TARGETS[label]
    X, w, row = me.sweep_population(d)
    mu, U = _bulk_whitening(d)
    target = me.place_outlier(X, row, mu, U, d, label)
    tr = _fit(X, w, me.SWEEP_SCALING[d])
    ymax, E, route = tr.x3_grid()
    if target is not None:
        assert abs(ymax / target - 1) < 1e-3, (ymax, target)
    assert E == E_want, (ymax, E)
    cap = gpu.mvn_x3_max_exponent()
    assert route == ("x3" if E <= cap else "f64"), (E, cap, route)
    assert tr._mfma and tr._prec == {"x3": 2, "f64": 0}[route]

    x, hint = _proposals(tr, me.SWEEP_M, _around(tr, X[row], N_NEAR, 7 * d), [row] * N_NEAR)
    ref = me.exact_mvn_logpdf(x, X, w, tr.cov)
    assert np.isfinite(ref).all()
    plain, hinted = _densities(tr, x, hint)
    e0, e1 = _rel(plain, ref), _rel(hinted, ref)
    b0, b1 = _bars(route)
    print(f"X3GRID sweep d={d} {label} ymax={ymax:.2f} E={E} route={route} "
          f"unhinted max {e0.max():.2e} median {np.median(e0):.2e} over {100 * (e0 > b0).mean():.1f}% | "
          f"hinted max {e1.max():.2e} median {np.median(e1):.2e} over {100 * (e1 > b1).mean():.1f}% | "
          f"around the outlier max {e0[-N_NEAR:].max():.2e} / {e1[-N_NEAR:].max():.2e}")
    assert not np.isnan(plain).any() and not np.isnan(hinted).any()
    assert e0.max() <= b0, (e0.max(), b0)
    assert e1.max() <= b1, (e1.max(), b1)


# ---- what does and does not move the grid ------------------------------------

@pytest.mark.parametrize("d", [2, 10])
def test_x3_zero_weight_outlier_moves_nothing(dev, d):
    """The E = 8 outlier with weight exactly 0: pop_range_kernel skips it, so
    the exponent stays where the bulk puts it, and neither the fit nor any
    density changes by a bit against the same population with that row in the
    bulk.  Candidates around the weightless row (hinted with it: an invalid
    hint) see the bulk alone, from ~160 kernel widths: the fp64 rescue."""
    X, w, row = me.sweep_population(d)
    w[row] = 0.0
    w /= w.sum()
    mu, U = _bulk_whitening(d)
    XA = X.copy()
    me.place_outlier(XA, row, mu, U, d, "E8-upper")
    trA, trB = _fit(XA, w), _fit(X, w)
    gA, gB = trA.x3_grid(), trB.x3_grid()
    assert gA == gB and gA[1] == 5 and gA[2] == "x3", (gA, gB)
    assert np.array_equal(trA.cov, trB.cov)
    far = _around(trA, XA[row], 4, 3)
    x, hint = _proposals(trB, me.SWEEP_M, far, [row] * 4)
    ref = me.exact_mvn_logpdf(x, XA, w, trA.cov)
    assert np.isfinite(ref).all() and (ref[-4:] < -1000).all()
    A0, A1 = _densities(trA, x, hint)
    B0, B1 = _densities(trB, x, hint)
    assert np.array_equal(A0.view(np.int64), B0.view(np.int64))
    assert np.array_equal(A1.view(np.int64), B1.view(np.int64))
    e0, e1 = _rel(A0[:-4], ref[:-4]), _rel(A1[:-4], ref[:-4])
    print(f"X3GRID zero-weight d={d} grid={gA} unhinted max {e0.max():.2e} hinted max {e1.max():.2e} "
          f"far rows |dlog| {np.abs(A0[-4:] - ref[-4:]).max():.1e}")
    assert e0.max() <= X3_TOL and e1.max() <= X3_TOL_HINTED
    np.testing.assert_allclose(A0[-4:], ref[-4:], rtol=RESCUE_RTOL, atol=0)
    np.testing.assert_allclose(A1[-4:], ref[-4:], rtol=RESCUE_RTOL, atol=0)


# ---- candidates at the norm bound ----------------------------------------------

def _bound_candidates(tr, X, E, seed):
    """8 directions x |z| = 2^E (1 -+ 1e-3, 1 -+ 1e-9): inside, outside and
    the hint of each (its nearest population row in the whitened metric)."""
    mu, U = _whitening(tr)
    rng = np.random.default_rng(seed)
    d = X.shape[1]
    fac = np.array([1 - 1e-3, 1 - 1e-9, 1 + 1e-9, 1 + 1e-3])
    x = np.array([me.point_at_norm(mu, U, v, 2.0 ** E * f)
                  for v in rng.standard_normal((8, d)) for f in fac])
    inside = np.tile(fac < 1, 8)
    z2 = me.whitened_norms(x, mu, U) ** 2
    assert (z2[inside] < 4.0 ** E).all() and (z2[~inside] > 4.0 ** E).all()
    Y = (X - mu) @ U
    hint = np.array([np.argmin((((xi - mu) @ U - Y) ** 2).sum(1)) for xi in x])
    return x, hint, inside


def _check_bound(tr, X, w, E, tag):
    xb, hb, inside = _bound_candidates(tr, X, E, 11 + E)
    x, hint = _proposals(tr, 200, xb, hb)
    inside = np.concatenate([np.ones(200, dtype=bool), inside])
    ref = me.exact_mvn_logpdf(x, X, w, tr.cov)
    assert np.isfinite(ref).all()
    plain, hinted = _densities(tr, x, hint)
    e0, e1 = _rel(plain, ref), _rel(hinted, ref)
    out = ~inside
    print(f"X3GRID bound {tag} E={E}: inside unhinted max {e0[inside].max():.2e} hinted max "
          f"{e1[inside].max():.2e}; at the bound (inside) {e0[200:][inside[200:]].max():.2e}; "
          f"outside |dlog|/|log| {np.abs(plain[out] / ref[out] - 1).max():.1e} / "
          f"{np.abs(hinted[out] / ref[out] - 1).max():.1e}; log density at the bound "
          f"{ref[200:].min():.0f} .. {ref[200:].max():.0f}")
    assert e0[inside].max() <= X3_TOL, e0[inside].max()
    assert e1[inside].max() <= X3_TOL_HINTED, e1[inside].max()
    np.testing.assert_allclose(plain[out], ref[out], rtol=RESCUE_RTOL, atol=0)
    np.testing.assert_allclose(hinted[out], ref[out], rtol=RESCUE_RTOL, atol=0)


def test_x3_norm_bound_smallest_exponent(dev):
    """E = 3 (d = 2, the kernel 20 x wider than Silverman's so that the
    population stays within one width): candidates with |z|^2 a relative 1e-9
    and 1e-3 inside 2^(2E) = 64 are answered by the kernel (~ -25 in log2
    against the -60 underflow bar) at the contract; those outside are flagged
    and rescued in fp64, 1e-9 in log density."""
    rng = np.random.default_rng(8)
    N, d = 1000, 2
    X = 0.5 + 0.8 * rng.standard_normal((N, d))
    w = np.exp(0.4 * rng.standard_normal(N))
    w /= w.sum()
    y1 = _fit(X, w).x3_grid()[0]
    want = 0.85 * me.exponent_interval(3, d)[1]
    tr = _fit(X, w, scaling=(y1 / want) ** 2)
    ymax, E, route = tr.x3_grid()
    assert E == 3 and route == "x3" and abs(ymax / want - 1) < 1e-6, (ymax, E, route)
    _check_bound(tr, X, w, 3, "d=2")


@pytest.mark.parametrize("d", [2, 10])
def test_x3_norm_bound_largest_exponent(dev, d):
    """The same at the largest exponent mvn_x3_kernel answers for, the
    outlier at that interval's upper edge.  Here a candidate at |z| = 2^E is
    at least 0.2 x 2^E from every particle, so inside the bound its density
    underflows the kernel's 2^-60 bar and it is rescued too: both sides take
    the fp64 path, the inside ones through the combine's underflow test and
    the outside ones through the pack's flag."""
    from pyabc_amd import gpu
    cap = gpu.mvn_x3_max_exponent()
    X, w, row = me.sweep_population(d)
    mu, U = _bulk_whitening(d)
    X[row] = me.point_at_norm(mu, U, me.outlier_direction(d, "E8-upper"),
                              me.target_norm(cap, "upper", d))
    tr = _fit(X, w, me.SWEEP_SCALING[d])
    ymax, E, route = tr.x3_grid()
    assert E == cap and route == "x3", (ymax, E, route)
    _check_bound(tr, X, w, cap, f"d={d}")


# ---- the ok == 0 image through the C ABI ------------------------------------------

def test_x3_image_past_the_cap_through_the_c_abi(dev):
    """abc_mvn_pack_population(X3) on a population past the cap writes an
    image marked not ok; abc_mvn_logpdf on that image flags every candidate
    and recomputes it in fp64 from the stored whitened population: finite, no
    NaN, 1e-9 in log density, unhinted and hinted (N = 500, M = 300, d = 5)."""
    import oracle
    from pyabc_amd import gpu
    from pyabc_amd import _native as nat
    from pyabc_amd.transition.multivariatenormal import psd_whitening
    rng = np.random.default_rng(15)
    N, M, d = 500, 300, 5
    cap = gpu.mvn_x3_max_exponent()
    X = 0.5 + 0.8 * rng.standard_normal((N, d))
    w = np.exp(0.4 * rng.standard_normal(N))
    w[7] = 1e-9 * w.sum()
    w /= w.sum()
    mu0, U0, _ = me.host_whitening(X, w)
    X[7] = me.point_at_norm(mu0, U0, rng.standard_normal(d),
                            1.05 * me.exponent_interval(cap, d)[1])
    cov, _ = oracle.mvn_fit(X, w)
    psd = psd_whitening(cov)
    assert psd["rank"] == d
    mu = w @ X
    shift = -np.log(w.max())
    log_norm = -0.5 * (d * np.log(2 * np.pi) + psd["log_pdet"])
    Xd, wd, mud, Ud = gpu.as_dev(X), gpu.as_dev(w), gpu.as_dev(mu), gpu.as_dev(psd["U"])
    packed, rng_d = gpu.mvn_pack(Xd, wd, mud, Ud, shift, nat.ABC_PREC_X3, with_range=True)
    ymax, E = rng_d.cpu().numpy()
    assert E == cap + 1, (ymax, E)
    anc = rng.integers(0, N, M)
    anc[:3] = 7
    x = X[anc] + 0.5 * rng.standard_normal((M, d)) @ np.linalg.cholesky(cov).T
    ref = me.exact_mvn_logpdf(x, X, w, cov)
    xd = gpu.as_dev(x)
    for hint in (None, gpu.as_dev(anc, dtype=torch.int64)):
        got = gpu.mvn_logpdf(xd, packed, N, mud, Ud, nat.ABC_PREC_X3, log_norm - shift,
                             X=Xd, w=wd, shift=shift, hint=hint).cpu().numpy()
        assert np.isfinite(got).all()
        print(f"X3GRID ok=0 image E={E:.0f} hinted={hint is not None}: "
              f"max |dlog| {np.abs(got - ref).max():.1e} max |dlog|/|log| "
              f"{np.abs(got / ref - 1).max():.1e}")
        np.testing.assert_allclose(got, ref, rtol=RESCUE_RTOL, atol=0)


# ---- shifted, scaled and correlated populations: the whole chain ---------------

@pytest.mark.parametrize("kind,d,a,b", me.chain_cases())
def test_mvn_chain_on_shifted_scaled_ridge_populations(dev, kind, d, a, b):
    """Moments, abc_mvn_fit, pack and density on offsets 1e4 / 1e6 with
    spreads 1e-2 / 1e-3, column scales 1e-6 .. 1e6 and rotated ridges of
    condition 1e4 .. 1e8.

    Covariance: ||L*^-1 (C - C*) L*^-T||_2 against the exact fit (integer
    sums, 40-digit factorisation) within 16 x what np.cov x Silverman^2 loses
    on the same input (both printed).  Density: the contract, against the
    exact reference evaluated with the reported covariance.  The column-scale
    population has eigenvalues below scipy's cut-off (rank 1 of 2, 4 of 10),
    so the transition answers with the direct fp64 kernel, as the reference
    implementation's frozen scipy distribution does; its bar is the f64 one."""
    X, w = me.chain_population(kind, d, a, b)
    tr = _fit(X, w)
    grid = tr.x3_grid()
    route = grid[2] if grid is not None else "direct"
    cov = tr.cov
    exact = me.exact_mvn_fit(X, w)
    bw2 = (4 / (1 / (w ** 2).sum()) / (d + 2)) ** (2 / (d + 4))
    e_np = le.whitened(np.cov(X, rowvar=False, aweights=w) * bw2, exact, 0)
    e_gpu = le.whitened(cov, exact, 0)
    x, hint = _proposals(tr, me.SWEEP_M)
    ref = me.exact_mvn_logpdf(x, X, w, cov)
    assert np.isfinite(ref).all()
    plain, hinted = _densities(tr, x, hint)
    e0, e1 = _rel(plain, ref), _rel(hinted, ref)
    print(f"X3GRID chain {kind} d={d} a={a:.0e} b={b:.0e} grid={grid} route={route} rank={tr._rank}: "
          f"cov whitened error kernel {e_gpu:.1e} np.cov {e_np:.1e} tol {16 * e_np:.1e} | "
          f"density unhinted max {e0.max():.2e} median {np.median(e0):.2e} "
          f"hinted max {e1.max():.2e} median {np.median(e1):.2e}")
    if kind == "scales":
        assert route == "direct" and tr._rank == {2: 1, 10: 4}[d]
    else:
        assert route == "x3" and tr._rank == d
    assert e_gpu <= 16 * e_np, (e_gpu, e_np)
    b0, b1 = _bars(route)
    assert e0.max() <= b0, (e0.max(), b0)
    assert e1.max() <= b1, (e1.max(), b1)
