"""LocalTransition fit and density on ill-conditioned populations: rotated
ridges (cond up to 1e8), two modes 30..300 apart, one stray particle.

Reference: oracle/local_exact.py (exact sums + 40-digit factorisations for
the fit, longdouble direct differences for the density).  Errors of the fit
are measured in the metric of the exact covariance (``whitened``), and the
tolerance is not a fixed number: 16 x what the float64 oracle itself loses on
the same rows, floored at 64 d eps.  A moments form that loses nothing beyond
its one-sweep centring stays within a small multiple of np.cov; one that
cancels against a far-away centre is 100x out or more
(tests/test_oracle_local_exact.py states both in float64 and asserts the
conditions on these inputs without a GPU).
"""
import numpy as np
import pytest

import oracle
from oracle import local_exact as le

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EPS = le.EPS64
LOG_2PI = np.log(2 * np.pi)


@pytest.fixture(scope="module")
def dev():
    from pyabc_amd import gpu
    return gpu.require_device()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def fit_errors(exact, covs, inv, chol=None, logdet=None):
    """Largest whitened error per quantity over the rows of ``exact``."""
    R = len(exact["rows"])
    out = dict(cov=max(le.whitened(covs[o], exact, o) for o in range(R)),
               inv=max(le.whitened_inv(inv[o], exact, o) for o in range(R)))
    if chol is not None:
        out["chol"] = max(le.whitened(chol[o] @ chol[o].T, exact, o) for o in range(R))
    if logdet is not None:
        out["logdet"] = float(np.abs(logdet - le.f64(exact["logdet"])).max())
    return out


def fmt(e):
    return " ".join(f"{k} {v:.1e}" for k, v in e.items())


@pytest.mark.parametrize("route,N,d,k,kappa,sep,stray", le.fit_cases())
def test_local_fit_conditioning(dev, route, N, d, k, kappa, sep, stray):
    """abc_local_fit on every moments route of launch_fit x ridge populations:
    covariance, inverse and Cholesky factor within tol = 16 x the oracle's own
    whitened error of the exact fit on 16 rows (ends of the ridge included),
    log det within d tol, log_norm consistent with dets, every output
    bit-identical across two calls, the EPS loop silent, and the route the
    case is meant for actually taken."""
    from pyabc_amd import gpu
    from pyabc_amd import _native as nat
    X, w, Q, rows = le.fit_case_inputs(N, d, k, kappa, sep, stray)
    exact = le.exact_local_fit(X, w, k, rows)
    ref = oracle.local_fit(X, w, k=k, k_fraction=None, rows=rows)
    Xd, wd = gpu.as_dev(X), gpu.as_dev(w)
    first = [t.cpu().numpy() for t in gpu.local_fit(Xd, wd, k, 1.0, 1e-3)]
    flags = gpu.local_fit_route()
    again = [t.cpu().numpy() for t in gpu.local_fit(Xd, wd, k, 1.0, 1e-3)]
    for name, a, b in zip(("covs", "inv_covs", "dets", "chol", "log_norm"), first, again):
        assert np.array_equal(bits(a), bits(b)), f"{name} differs between two calls"
    covs, inv, dets, chol, lnorm = (a[rows] for a in first)

    e_ref = fit_errors(exact, ref["covs"], ref["inv_covs"])
    e_gpu = fit_errors(exact, covs, inv, chol, np.log(dets))
    tol = max(16 * max(e_ref.values()), 64 * d * EPS)
    names = gpu.local_fit_route_names(flags)
    msg = (f"{route} N={N} d={d} k={k} kappa={kappa:.0e} sep={sep} stray={stray} "
           f"route={names}: oracle {fmt(e_ref)} | kernel {fmt(e_gpu)} | tol {tol:.1e}")
    print("FIT " + msg)

    Cstar = le.f64(exact["C"])
    assert np.abs(covs - Cstar).max() < 5e-4, \
        "the 'while det <= 0: cov += EPS I' loop fired on a positive definite fit: " + msg
    assert (dets > 0).all(), msg
    assert e_gpu["cov"] <= tol, msg
    assert e_gpu["inv"] <= tol, msg
    assert e_gpu["chol"] <= tol, msg
    assert e_gpu["logdet"] <= d * tol, msg
    assert np.array_equal(np.triu(chol, 1), np.zeros_like(chol)), "chol not lower triangular"
    np.testing.assert_allclose(lnorm, 0.5 * (d * LOG_2PI + np.log(dets)), rtol=0, atol=1e-14)

    if route in le.DENSE_ROUTES and (kappa, sep, stray) == (1e4, 0, None):
        assert flags & nat.ABC_FIT_DENSE and not flags & nat.ABC_FIT_DENSE_REJECTED, msg
    if stray == 1e4:
        assert flags & nat.ABC_FIT_DENSE_REJECTED, msg
    if route == "wide-control":
        assert flags == 0, msg


@pytest.mark.parametrize("d,N,M,kappa,sep,scale,stray,stray_row", le.pdf_cases())
def test_local_logpdf_conditioning(dev, d, N, M, kappa, sep, scale, stray, stray_row):
    """abc_local_logpdf against the exact log density, the fit taken from the
    extended-precision fit rounded to float64 (the density alone is under
    test): absolute 2e-6 wherever the exact value is >= -700, <= -699 below.
    Ridges with the modes 30 and 300 apart, and a well-conditioned bulk (local
    covariances ~0.03) with one stray particle at row 0 -- the row the packed
    form is centred at -- or at row N-1, where it must not matter either."""
    from pyabc_amd import gpu
    c = le.pdf_case_inputs(d, N, M, kappa, sep, scale, stray, stray_row)
    exact = le.exact_local_logpdf(c["x"], c["X"], c["w"], c["inv"], c["lnorm"])
    got = gpu.local_logpdf(gpu.as_dev(c["x"]), gpu.as_dev(c["X"]), gpu.as_dev(c["w"]),
                           gpu.as_dev(c["inv"]), gpu.as_dev(c["lnorm"])).cpu().numpy()
    ndirect, bound = gpu.local_logpdf_route(M, N, d)
    cmp_ = exact >= -700
    assert not cmp_[0] and cmp_.sum() >= M // 2
    err = np.abs(got[cmp_] - exact[cmp_]).max()
    print(f"PDF d={d} N={N} M={M} kappa={kappa:.0e} sep={sep} stray={stray} "
          f"row={stray_row}: max |log density error| {err:.1e} on {cmp_.sum()} candidates, "
          f"{ndirect} of {M} by the direct form (bound at X_0 {bound:.1e})")
    # the cases cannot pass by always taking the direct form (here only the
    # far candidate does), nor the stray ones by luck on the expanded form
    if (kappa, sep, stray) == (1e4, 0, None) and d <= 5:
        assert ndirect == 1, (ndirect, bound)
    if stray is not None and stray >= 1e4:
        assert ndirect == M, (ndirect, bound)
    assert not np.isnan(got).any()
    assert (got[~cmp_] <= -699).all(), got[~cmp_]
    assert err <= 2e-6, err


@pytest.mark.parametrize("sep", [0, 30])
def test_local_transition_fit_then_pdf_on_a_ridge(dev, sep):
    """LocalTransition.fit then .pdf through the Python class at d = 3,
    N = 3000, default k = N/4, kappa = 1e6, against the exact fit followed by
    the exact density.  sep = 0 (one mode) is the fast composition: the dense
    deferred moments accepted by their rounding guard, feeding the packed
    MFMA density -- both asserted.  sep = 30 (two modes 30 apart) is the
    careful one: the guard rejects the dense moments, so the fit comes from
    the VALU sweep, and the density's expansion bound sends the candidates to
    the direct form.  Bar: the density's 2e-6 plus what the fit's tolerance
    allows the Mahalanobis form to move, 0.5 q_max tol (q_max the largest
    q_ij among the terms that take part in a compared value; tol as in
    test_local_fit_conditioning, measured on 16 rows)."""
    import pandas as pd
    from pyabc_amd import gpu
    from pyabc_amd import _native as nat
    from pyabc_amd.transition import LocalTransition
    N, d, kappa = 3000, 3, 1e6
    X, w, Q = le.ridge_population(N, d, kappa, sep, seed=3000)
    cols = [f"p{a}" for a in range(d)]
    t = LocalTransition()
    t.fit(pd.DataFrame(X, columns=cols), w.copy())
    flags = gpu.local_fit_route()
    route = gpu.local_fit_route_names(flags)
    k = t.k
    assert k == N // 4
    rows = le.check_rows(X, Q, 3000)
    exact = le.exact_local_fit(X, w, k, rows)
    ref = oracle.local_fit(X, w, k=k, k_fraction=None, rows=rows)
    e_ref = fit_errors(exact, ref["covs"], ref["inv_covs"])
    tol = max(16 * max(e_ref.values()), 64 * d * EPS)
    # every row's fit for the density (longdouble: 2^-63 cond from exact, far
    # inside tol)
    full = le.exact_local_fit(X, w, k, np.arange(N),
                              method="longdouble" if le.LONGDOUBLE_OK else "exact")
    rng = np.random.default_rng(11)
    r = rng.integers(0, N, 64)
    L = le.f64(full["L"])
    x = X[r] + 0.3 * np.einsum("mab,mb->ma", L[r], rng.standard_normal((64, d)))
    xp = full["xp"]
    lnorm = 0.5 * (d * xp.log(xp.arr(2 * np.pi)) + full["logdet"])
    want, q = le.exact_local_logpdf(x, X, w, full["A"], lnorm, with_q=True)
    got = np.log(np.asarray(t.pdf(pd.DataFrame(x, columns=cols))))
    assert (want >= -700).all()
    bar = 2e-6 + 0.5 * q.max() * tol
    err = np.abs(got - want).max()
    ndirect, bound = gpu.local_logpdf_route(64, N, d)
    print(f"COMPOSED sep={sep} fit route={route}, {ndirect} of 64 candidates by the direct form "
          f"(bound at X_0 {bound:.1e}) k={k} oracle {fmt(e_ref)} tol {tol:.1e} q_max {q.max():.1f} "
          f"bar {bar:.2e} err {err:.2e}")
    assert err <= bar, (err, bar)
    assert flags & nat.ABC_FIT_DENSE and flags & nat.ABC_FIT_DEFER, route
    if sep == 0:
        assert not flags & nat.ABC_FIT_DENSE_REJECTED, route
        assert ndirect <= 8, (ndirect, bound)
    else:
        assert flags & nat.ABC_FIT_DENSE_REJECTED, route
        assert ndirect == 64, (ndirect, bound)
