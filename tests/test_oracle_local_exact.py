"""The extended-precision LocalTransition reference (oracle/local_exact.py),
the conditions on the inputs of tests/test_gpu_local_conditioning.py, and
float64 emulations of the three moments forms and of the expanded density
form that say why those inputs were chosen.  No GPU: numpy and mpmath only.
"""
import numpy as np
import pytest

import oracle
from oracle import local_exact as le

EPS = le.EPS64


# ---- the reference itself ----------------------------------------------------

def test_exact_fit_matches_mpmath_two_pass():
    """Exact integer sums + 40-digit factorisations against the two-pass form
    evaluated at 40 digits throughout: 1e-17 whitened on 3 rows of a
    kappa = 1e8 case (both are ~1e-40 cond out; the two share no summation)."""
    N, d, k = 1500, 3, 400
    X, w, Q, rows = le.fit_case_inputs(N, d, k, 1e8, 30, None)
    rows = rows[[0, 5, -1]]
    fe = le.exact_local_fit(X, w, k, rows)
    fm = le.exact_local_fit(X, w, k, rows, method="mpmath")
    for o in range(3):
        assert le.whitened(fe["C"][o], fm, o) <= 1e-17
        assert le.whitened_inv(fe["A"][o], fm, o) <= 1e-17
        assert le.whitened(fe["L"][o] @ fe["L"][o].T, fm, o) <= 1e-17
        assert abs(float(fe["logdet"][o] - fm["logdet"][o])) <= 1e-17
        assert np.array_equal(fe["nb"][o], fm["nb"][o])


@pytest.mark.skipif(not le.LONGDOUBLE_OK, reason="longdouble is not 80-bit here")
def test_longdouble_fit_is_eps_cond_from_exact():
    """The longdouble two-pass fit (the density tests' fit) is within
    16 * 2^-63 * cond(C*) of the exact one -- and not much better: entrywise
    rounding of C* to a 64-bit mantissa is already of that order, which is
    why the fit tests' reference is not longdouble."""
    N, d, k = 1500, 3, 400
    X, w, Q, rows = le.fit_case_inputs(N, d, k, 1e8, 30, None)
    rows = rows[[0, 5, -1]]
    fe = le.exact_local_fit(X, w, k, rows)
    fl = le.exact_local_fit(X, w, k, rows, method="longdouble")
    eld = float(np.finfo(np.longdouble).eps)
    worst = 0.0
    for o in range(3):
        cond = np.linalg.cond(le.f64(fe["C"][o]))
        e = max(le.whitened(fl["C"][o], fe, o), le.whitened_inv(fl["A"][o], fe, o))
        assert e <= 16 * eld * cond, (e, cond)
        worst = max(worst, e / (eld * cond))
    assert worst > 1e-3, worst


def test_exact_logpdf_matches_mpmath():
    """Longdouble direct-difference log-sum-exp against the same at 40 digits
    (kappa = 1e8, d = 2, a far candidate included: no exp underflow)."""
    c = le.pdf_case_inputs(2, 601, 130, 1e8, 30, 1.0, None, 0)
    x = c["x"][[0, 1, 2, 77]]
    a = le.exact_local_logpdf(x, c["X"], c["w"], c["inv"], c["lnorm"])
    b = le.exact_local_logpdf(x, c["X"], c["w"], c["inv"], c["lnorm"],
                              xp=le.backend("mpmath"))
    assert np.isfinite(a).all() and a[0] < -1e6
    np.testing.assert_allclose(a[1:], b[1:], rtol=0, atol=1e-9)
    np.testing.assert_allclose(a[0], b[0], rtol=1e-12)


def test_exact_fit_equals_oracle_on_a_benign_population():
    """On a well-conditioned population the exact fit is the oracle's."""
    rng = np.random.default_rng(5)
    X = rng.normal(size=(300, 4))
    w = rng.random(300)
    rows = np.array([0, 17, 299])
    f = le.exact_local_fit(X, w, 30, rows)
    ref = oracle.local_fit(X, w, k=30, k_fraction=None, rows=rows)
    np.testing.assert_allclose(le.f64(f["C"]), ref["covs"], rtol=1e-12)
    np.testing.assert_allclose(le.f64(f["A"]), ref["inv_covs"], rtol=1e-11)
    np.testing.assert_allclose(np.exp(le.f64(f["logdet"])), ref["dets"], rtol=1e-12)


# ---- conditions on the GPU tests' inputs --------------------------------------
# (conditions on the inputs, not tolerances for a kernel: seeds and rows are
# chosen so that they hold)

@pytest.mark.parametrize("route,N,d,k,kappa,sep,stray", le.fit_cases())
def test_fit_case_inputs(route, N, d, k, kappa, sep, stray):
    X, w, Q, rows = le.fit_case_inputs(N, d, k, kappa, sep, stray)
    assert len(rows) == 16 and rows[0] == 0 and rows[-1] == N - 1
    fit = le.exact_local_fit(X, w, k, rows)       # raises unless det C* > 0
    ref = oracle.local_fit(X, w, k=k, k_fraction=None, rows=rows)
    # the neighbour set does not hang on the last bit of a distance
    assert fit["gap"].min() > 1e-10, fit["gap"].min()
    assert np.isfinite(le.f64(fit["logdet"])).all()
    worst = 0.0
    for o in range(len(rows)):
        cond = np.linalg.cond(le.f64(fit["C"][o]))
        assert cond <= 1e9, (rows[o], cond)
        e = max(le.whitened(ref["covs"][o], fit, o),
                le.whitened_inv(ref["inv_covs"][o], fit, o))
        assert e <= 16 * EPS * cond, (rows[o], e, cond)
        worst = max(worst, e / (EPS * cond))
    print(f"oracle whitened error / (eps cond) <= {worst:.2f}")


@pytest.mark.parametrize("d,N,M,kappa,sep,scale,stray,stray_row", le.pdf_cases())
def test_pdf_case_inputs(d, N, M, kappa, sep, scale, stray, stray_row):
    """The float64 oracle, given the same fit, is within 5e-7 of the exact log
    density on every compared candidate: a quarter of the kernel's 2e-6."""
    c = le.pdf_case_inputs(d, N, M, kappa, sep, scale, stray, stray_row)
    exact = le.exact_local_logpdf(c["x"], c["X"], c["w"], c["inv"], c["lnorm"])
    fit = dict(w=c["w"], inv_covs=c["inv"], normalization=np.exp(c["lnorm"]))
    got = oracle.local_logpdf(c["x"], c["X"], fit)
    cmp_ = exact >= -700
    assert exact[0] < -700 and cmp_[1:].sum() >= M // 2, cmp_.sum()
    err = np.abs(got[cmp_] - exact[cmp_]).max()
    print(f"oracle log-density error {err:.1e} on {cmp_.sum()} candidates")
    assert err <= 5e-7, err


# ---- why these inputs: the three moments forms in float64 ---------------------

def _finish(S0, Q, S1, S2):
    """local_finish_kernel's covariance from sums about the particle."""
    mean = S1 / S0
    return (S2 / S0 - np.outer(mean, mean)) / (1.0 - Q / (S0 * S0))


def form_np_cov(X, w, n, nb):
    """The oracle's form: np.cov(aweights) of the offsets (two passes)."""
    return oracle.smart_cov(X[nb] - X[n], w[nb] / w[nb].sum())


def form_one_sweep(X, w, n, nb):
    """local_moments_kernel / knn_select_kernel's list mode: raw sums of the
    offsets about X_n in one sweep, centred afterwards."""
    D, lw = X[nb] - X[n], w[nb]
    return _finish(lw.sum(), (lw * lw).sum(), lw @ D, (D * lw[:, None]).T @ D)


def form_recentred(X, w, n, nb):
    """The dense path: raw sums about X_0 (taken exactly here: the limb
    rounding is left out, the best case for this form), re-centred at X_n in
    float64 as mm_finish_kernel does, ((S - t1) - t2) + t3."""
    Xi, ex = le._exact_ints(X)
    wi, ew = le._exact_ints(w)
    Y, lw = Xi[nb] - Xi[0], wi[nb]
    sx, sw = 2.0 ** ex, 2.0 ** ew
    S0 = float(lw.sum()) * sw
    Q = float((lw * lw).sum()) * sw * sw
    S1 = np.array([float(v) for v in (lw[:, None] * Y).sum(0)]) * sw * sx
    S2i = ((lw[:, None] * Y).T[:, None, :] * Y.T[None, :, :]).sum(2)
    S2 = np.array([[float(v) for v in r] for r in S2i]) * sw * sx * sx
    yn = X[n] - X[0]
    m1 = S1 - S0 * yn
    d = len(yn)
    M2 = np.empty((d, d))
    for a in range(d):
        for b in range(d):
            t1, t2, t3 = S1[a] * yn[b], S1[b] * yn[a], S0 * yn[a] * yn[b]
            M2[a, b] = ((S2[a, b] - t1) - t2) + t3
    return _finish(S0, Q, m1, M2)


FORMS = (form_np_cov, form_one_sweep, form_recentred)


def moments_forms_errors(d, k, kappa, sep, N=3000, nrows=4):
    X, w, Q = le.ridge_population(N, d, kappa, sep, seed=int(d + k + sep))
    rows = np.array([N // 2 + 5, N - N // 5, N - 1,
                     int((X @ Q[:, 0]).argmax())])[:nrows]
    fit = le.exact_local_fit(X, w, k, rows)
    return [max(le.whitened(f(X, w, int(n), fit["nb"][o]), fit, o)
                for o, n in enumerate(rows)) for f in FORMS]


@pytest.mark.parametrize("d,k,kappa,sep,dense_over_ref", [
    (3, 700, 1.0, 30, None), (3, 700, 1e6, 0, None), (3, 700, 1e6, 30, 30.0),
    (3, 700, 1e8, 30, 30.0), (2, 400, 1e8, 30, 30.0)])
def test_emulated_moments_forms(d, k, kappa, sep, dense_over_ref):
    """Whitened covariance error of the three forms, rows of the far mode
    (|X_n - X_0| ~ sep), the far end of the ridge among them.  The form
    re-centred from X_0 is more than 30x np.cov once the modes are 30 apart
    and the ridge is thin (its cancellation is sized by |X_n - X_0|^2, the
    local variance in the thin direction by 1 / kappa).  The one-sweep form
    is within 16x at kappa = 1e6, sep = 30; its extra factor is 1 + |mean
    offset|^2 / variance, and the particle at the end of a d = 2 ridge, whose
    neighbours all lie to one side, reaches 30x at kappa = 1e8."""
    ref, sweep, dense = moments_forms_errors(d, k, kappa, sep)
    print(f"np.cov {ref:.1e}  one sweep {sweep:.1e}  re-centred {dense:.1e}")
    assert sweep <= (16 if kappa <= 1e6 else 100) * max(ref, 64 * d * EPS)
    if dense_over_ref is not None:
        assert dense > dense_over_ref * ref
    else:
        # one mode or a round ridge: the re-centring costs little
        assert dense <= 100 * max(ref, 64 * d * EPS)


# ---- why these inputs: the expanded density form in float64 -------------------

def expanded_q(x, X, inv):
    """q_ij as local_pack_kernel / local_mfma_kernel form it: the quadratic
    form expanded in coordinates centred at X_0, psi_j . phi(y_i)."""
    Y, y = X - X[0], x - X[0]
    As = 0.5 * (inv + inv.transpose(0, 2, 1))
    lin = np.einsum("jab,jb->ja", As, Y)             # (A_s Y_j)
    const = np.einsum("ja,ja->j", Y, np.einsum("jab,jb->ja", inv, Y))
    quad = np.einsum("ia,jab,ib->ij", y, As, y)
    return quad - 2.0 * (y @ lin.T) + const[None, :]


def direct_q(x, X, inv, dtype):
    D = X.astype(dtype)[None, :, :] - x.astype(dtype)[:, None, :]
    A = inv.astype(dtype)
    return ((D[:, :, :, None] * A[None]).sum(2) * D).sum(2)


def density_forms_errors(d, kappa, sep, scale, stray, N=600, M=40):
    c = le.pdf_case_inputs(d, N, M, kappa, sep, scale, stray, 0)
    x = c["x"][1:]
    exact = direct_q(x, c["X"], c["inv"], np.longdouble)
    near = exact < 100
    e_dir = np.abs(direct_q(x, c["X"], c["inv"], np.float64) - exact)[near].max() / 2
    e_exp = np.abs(expanded_q(x, c["X"], c["inv"]) - exact)[near].max() / 2
    return float(e_dir), float(e_exp)


@pytest.mark.skipif(not le.LONGDOUBLE_OK, reason="longdouble is not 80-bit here")
@pytest.mark.parametrize("d,kappa,sep,scale,stray,red", [
    (5, 1e6, 30, 1.0, None, False), (5, 1e6, 300, 1.0, None, True),
    (2, 1e8, 30, 1.0, None, True), (5, 1e8, 30, 1.0, None, None),
    (3, 1.0, 0, 0.3, 1e4, True), (5, 1.0, 0, 0.3, 1e4, True)])
def test_emulated_density_forms(d, kappa, sep, scale, stray, red):
    """Absolute error of q_ij / 2 (the log-density term) over pairs with
    q < 100.  The direct form (the oracle's) stays below the 5e-7 the input
    conditions allow; the form expanded about row 0 rounds at
    eps |A_j| |y|^2 and crosses the kernel's 2e-6 bar where the modes are far
    apart on a thin ridge, or where row 0 is a stray particle (red; None: at
    the bar, 1.3e-6 on these 39 candidates)."""
    e_dir, e_exp = density_forms_errors(d, kappa, sep, scale, stray)
    print(f"direct {e_dir:.1e}  expanded about X_0 {e_exp:.1e}")
    assert e_dir <= 5e-7
    assert e_exp > 8 * e_dir
    if red is not False:
        assert e_exp > (2e-6 if red else 5e-7)
