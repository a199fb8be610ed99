"""Extended-precision MultivariateNormalTransition reference, and the
populations that aim the x3 density kernel at a chosen limb-grid exponent.

Test infrastructure only -- see ``oracle/__init__.py``.

``oracle.mvn_logpdf`` is float64 and whitens ``X @ U`` and ``x @ U`` before it
subtracts: on a population at offset 1e6 with spread 1e-3 the whitened
coordinates are ~2e9 and their differences carry ~4e-7, which is the size of
what a test of the kernels wants to measure.  The functions here take the
direct differences x_i - X_j first, whiten them with a factor of the reported
covariance computed at 40 digits (mpmath Cholesky: ``local_exact``'s helpers)
and reduce with a log-sum-exp, all in 80-bit longdouble (mpmath where a
longdouble is not 80-bit).  The fit is restated from exact integer sums, as
``local_exact.exact_local_fit`` does for one neighbourhood.
"""
import numpy as np

from . import local_exact as le

SQRT_LOG2E = 1.2011224087864498      # the x3 kernel's coordinate scale
E_MIN = 3


def _mp_to_xp(xp, v):
    """An mpmath number in the density backend's number type."""
    if xp.name == "mpmath":
        return v
    hi = float(v)
    return np.longdouble(hi) + np.longdouble(float(v - hi))


def exact_whitening(cov):
    """The float64 covariance taken as an exact input: its Cholesky factor L,
    L^-1 and log det at 40 digits.  Laid out as one row of an
    ``exact_local_fit`` (leading axis 1) so that ``local_exact.whitened``
    measures a covariance against it."""
    xp = le.backend("mpmath")
    C = xp.arr(np.atleast_2d(np.asarray(cov, dtype=np.float64)))
    return _factorise(xp, C)


def _factorise(xp, C):
    L = le._cholesky(xp, C)
    Li = le._lower_inverse(xp, L)
    return dict(C=C[None], L=L[None], Linv=Li[None], LT=L.T[None],
                logdet=2 * xp.log(np.diagonal(L)).sum(), xp=xp)


def exact_mvn_fit(X, w, scaling=1.0):
    """MultivariateNormalTransition.fit beyond float64: C* = np.cov(X,
    aweights=w) x silverman(ESS, d)^2 x scaling.  The float64 inputs are
    integers times a power of two, so S0 = sum w, S1 = sum w x, S2 = sum w x
    x^T, Q = sum w^2 are summed exactly in Python integers and the covariance
    (S0 S2 - S1 S1^T) / (S0^2 - Q) is one exact ratio per entry, whatever the
    population's offset; ESS = S0^2 / Q.  The bandwidth power and the d x d
    factorisation round at 40 digits.  Returns the layout of
    ``exact_whitening``."""
    xp = le.backend("mpmath")
    mpf = xp.mp.mpf
    X64 = np.asarray(X, dtype=np.float64)
    N, d = X64.shape
    Xe, ex = le._exact_ints(X64)
    we, _ = le._exact_ints(np.asarray(w, dtype=np.float64))
    wX = we[:, None] * Xe
    S0, S1, Q = we.sum(), wX.sum(0), (we * we).sum()
    S2 = np.dot(wX.T, Xe)
    num = S0 * S2 - S1[:, None] * S1[None, :]
    ess = mpf(int(S0 * S0)) / mpf(int(Q))
    bw2 = (4 / ess / (d + 2)) ** (mpf(2) / (d + 4))
    scale = mpf(2) ** (2 * ex) / mpf(int(S0 * S0 - Q)) * bw2 * mpf(float(scaling))
    C = np.array([[mpf(int(v)) * scale for v in r] for r in num], dtype=object)
    return _factorise(xp, C)


def exact_psd(cov):
    """scipy.stats._multivariate._PSD on the float64 covariance taken as an
    exact input, its eigen-decomposition at 40 digits (mpmath eigsy): the
    eigenvalues, which of them pass the cut-off 1e6 eps max|s|, and -- only
    where some do not -- the whitening U = u / sqrt(s) of the kept ones, the
    null-space basis V, log pdet and the support tolerance, as
    ``oracle.psd_decompose`` states them in float64."""
    xp = le.backend("mpmath")
    mp = xp.mp
    C = np.atleast_2d(np.asarray(cov, dtype=np.float64))
    d = C.shape[0]
    E, Q = mp.eigsy(mp.matrix(C.tolist()))
    s = np.array([E[a] for a in range(d)], dtype=object)
    cut = 1e6 * le.EPS64 * float(max(abs(v) for v in s))
    keep = np.array([bool(v > cut) for v in s])
    out = dict(s=s, keep=keep, rank=int(keep.sum()), support_tol=1e3 * cut, xp=xp)
    if not keep.all():
        u = np.array([[Q[a, b] for b in range(d)] for a in range(d)], dtype=object)
        out["U"] = u[:, keep] / xp.sqrt(s[keep])[None, :]
        out["V"] = u[:, ~keep]
        out["log_pdet"] = xp.log(s[keep]).sum()
    return out


def exact_mvn_logpdf(x, X, w, cov, screen=60.0, xp=None):
    """log sum_j w_j N(x_i - X_j; 0, cov) with direct differences first, then
    the whitening, then a log-sum-exp, in extended precision; w as given (not
    normalised), rows with w = 0 left out.  Returns float64.

    The whitening is T = L^-1 of ``exact_whitening(cov)`` (|T d|^2 = d^T
    cov^-1 d).  A covariance with eigenvalues below scipy's cut-off (which the
    transition evaluates as scipy's frozen ``multivariate_normal(cov,
    allow_singular=True)`` does) takes T = U^T of ``exact_psd`` instead, the
    pseudo-determinant, and density 0 for the pairs whose difference leaves
    the support, |d V| >= support_tol.

    screen: terms more than this many nats below a candidate's largest (both
    from a float64 direct-difference pass, good to far better than a nat) are
    left out of the extended-precision sum: N e^-60 < 1e-22 relative at the
    N <= 1e4 of the tests, and most pairs of a 10-D population go.  None
    keeps every term."""
    xp = xp or le.backend()
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    X = np.asarray(X, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    d = X.shape[1]
    psd = exact_psd(cov)
    mp = psd["xp"].mp
    if psd["rank"] == d:
        fit = exact_whitening(cov)
        Tm, logdet, Vm = fit["Linv"][0], fit["logdet"], None
    else:
        Tm, logdet, Vm = psd["U"].T, psd["log_pdet"], psd["V"]
    conv = (lambda a: a) if xp.name == "mpmath" else le._ld
    T, T64 = conv(Tm), le.f64(Tm)
    V, V64 = (None, None) if Vm is None else (conv(Vm), le.f64(Vm))
    norm = _mp_to_xp(xp, -(psd["rank"] * mp.log(2 * mp.pi) + logdet) / 2)
    keep = w > 0
    Xk = X[keep]
    Xe = xp.arr(Xk)
    logw = xp.log(xp.arr(w[keep]))
    logw64 = le.f64(logw)
    out = np.empty(len(x))
    for i in range(len(x)):
        if screen is None:
            sel = np.ones(len(Xk), dtype=bool)
        else:
            Z64 = (x[i] - Xk) @ T64.T
            t64 = logw64 - 0.5 * (Z64 * Z64).sum(1)
            if V is not None:   # screen among the pairs (nearly) in the support
                R64 = (x[i] - Xk) @ V64
                t64[np.sqrt((R64 * R64).sum(1)) >= 2 * psd["support_tol"]] = -np.inf
            sel = t64 >= t64.max() - screen
        D = xp.arr(x[i]) - Xe[sel]
        Z = np.dot(D, T.T)
        t = logw[sel] - (Z * Z).sum(1) / 2
        if V is not None:
            R = np.dot(D, V)
            t = t[le.f64(xp.sqrt((R * R).sum(1))) < psd["support_tol"]]
        if len(t) == 0:
            out[i] = -np.inf
            continue
        m = t.max()
        out[i] = float(m + xp.log(xp.exp(t - m).sum()) + norm)
    return out


# ---- the x3 kernel's grid exponent, restated on the host ---------------------

def grid_exponent(ymax, r):
    """x3_setup_kernel: E = max(3, ceil(log2(1.25 max|y| + 2 sqrt(r) + 4)))."""
    return max(E_MIN, int(np.ceil(np.log2(1.25 * ymax + 2.0 * np.sqrt(r) + 4.0))))


def exponent_interval(E, r):
    """(lo, hi]: the largest whitened norms max|y| that give grid exponent E
    at rank r (lo = 0 at E = 3)."""
    off = 2.0 * np.sqrt(r) + 4.0
    lo = 0.0 if E <= E_MIN else max((2.0 ** (E - 1) - off) / 1.25, 0.0)
    return lo, (2.0 ** E - off) / 1.25


def whitened_norms(X, mu, U):
    """|y_j| in the kernel's units: y = sqrt(log2 e) (X - mu) U."""
    Y = (np.asarray(X) - mu) @ U
    return SQRT_LOG2E * np.sqrt((Y * Y).sum(1))


def point_at_norm(mu, U, v, norm):
    """The point x with sqrt(log2 e) (x - mu) U = norm v / |v| (U square,
    full rank)."""
    v = np.asarray(v, dtype=np.float64)
    y = v / np.linalg.norm(v) * (norm / SQRT_LOG2E)
    return mu + np.linalg.solve(U.T, y)


def host_whitening(X, w, scaling=1.0):
    """Float64 fit on the host (np.cov semantics, Silverman): mean, a square
    whitening U with U U^T = cov^-1, cov.  What the CPU tests place points
    with; the GPU tests take the device fit's own mu and U."""
    import oracle
    cov, wn = oracle.mvn_fit(X, w, scaling=scaling)
    mu = wn @ np.asarray(X, dtype=np.float64)
    U = np.linalg.inv(np.linalg.cholesky(cov)).T
    return mu, U, cov


# ---- the cases of tests/test_gpu_x3_grid.py ----------------------------------
# (shared with tests/test_oracle_mvn_exact.py, which asserts the conditions on
# these inputs without a GPU)

SWEEP_N = 3000
SWEEP_M = 400
SWEEP_DIMS = (1, 2, 10, 25)
OUTLIER_WEIGHT = 1e-9
# label -> (E aimed at, where in that E's interval the outlier's norm sits)
SWEEP_TARGETS = {
    "E5": (5, None),             # no outlier: the bulk alone
    "E6": (6, "mid"),
    "E6-upper": (6, "upper"),
    "E7-lower": (7, "lower"),
    "E7-upper": (7, "upper"),
    "E8-lower": (8, "lower"),
    "E8-upper": (8, "upper"),
    "E9": (9, "past"),           # just past the E = 8 edge
}
# transition scaling per dimension: 1 where the Gaussian bulk of 3000 lands
# inside the E = 5 interval by itself; at d = 25 the bulk's largest norm
# (~13) sits within a few percent of the E = 5 / 6 edge (14.4), and the wider
# kernel moves it to the middle of the interval
SWEEP_SCALING = {1: 1.0, 2: 1.0, 10: 1.0, 25: 1.5}


def target_norm(E, where, r):
    """The outlier's whitened norm for a target: 3 % above the interval's
    lower edge (1 % for "past"), 1 % below its upper edge, or its middle
    (r = 10: 44 and 93 for E = 7, 97 and 195 for E = 8, 198.5 for E = 9)."""
    lo, hi = exponent_interval(E, r)
    return {"lower": 1.03 * lo, "past": 1.01 * lo, "upper": 0.99 * hi,
            "mid": 0.5 * (lo + hi)}[where]


def sweep_cases():
    return [(d, label) for d in SWEEP_DIMS for label in SWEEP_TARGETS]


def sweep_population(d, N=SWEEP_N, outlier_weight=OUTLIER_WEIGHT):
    """Gaussian bulk (mean 0.5, spread 0.8, weights exp(0.4 normal)) whose row
    ``row`` carries ``outlier_weight`` of the total; the row starts at a bulk
    position (no outlier) and is moved by the caller.  Returns X, w
    (normalised), row."""
    rng = np.random.default_rng(4000 + d)
    X = 0.5 + 0.8 * rng.standard_normal((N, d))
    w = np.exp(0.4 * rng.standard_normal(N))
    row = N // 3
    w[row] = 0.0
    w[row] = outlier_weight * w.sum()
    w /= w.sum()
    return X, w, row


def outlier_direction(d, label):
    rng = np.random.default_rng(97 * d + sorted(SWEEP_TARGETS).index(label))
    return rng.standard_normal(d)


def place_outlier(X, row, mu, U, d, label):
    """Move the outlier row of a sweep population to its target norm along the
    case's direction, in the whitening (mu, U) given.  Returns the target
    norm (None: no outlier)."""
    E, where = SWEEP_TARGETS[label]
    if where is None:
        return None
    norm = target_norm(E, where, d)
    X[row] = point_at_norm(mu, U, outlier_direction(d, label), norm)
    return norm


# offset populations: X = offset + spread * normal
OFFSET_CASES = [(off, spread) for off in (1e4, 1e6) for spread in (1e-2, 1e-3)]
RIDGE_KAPPAS = (1e4, 1e6, 1e8)
CHAIN_DIMS = (2, 10)


def chain_cases():
    """(kind, d, a, b): offset (a = offset, b = spread), scales (columns
    1e-6 .. 1e6), ridge (a = kappa)."""
    out = []
    for d in CHAIN_DIMS:
        out += [("offset", d, off, sp) for (off, sp) in OFFSET_CASES]
        out.append(("scales", d, 1e-6, 1e6))
        out += [("ridge", d, k, 0.0) for k in RIDGE_KAPPAS]
    return out


def chain_population(kind, d, a, b, N=SWEEP_N):
    """Population and normalised weights of a chain case."""
    seed = int(500 + 13 * d + np.log10(a) * 7 + (np.log10(b) if b > 0 else 0))
    rng = np.random.default_rng(seed)
    if kind == "ridge":
        X, w, _ = le.ridge_population(N, d, a, 0, seed)
        return X, w
    G = rng.standard_normal((N, d))
    if kind == "offset":
        # correlated unit-order bulk, then the spread and the offset
        A = np.eye(d) + 0.3 * rng.standard_normal((d, d)) / np.sqrt(d)
        X = a + b * (G @ A.T)
    else:
        X = (0.3 + G) * np.logspace(np.log10(a), np.log10(b), d)
    w = np.exp(0.4 * rng.standard_normal(N))
    return X, w / w.sum()


def chain_candidates(X, cov, M=SWEEP_M, seed=0):
    """Candidates 0.5 kernel widths around random ancestors (the ancestors
    are the hints).  Returns x, anc."""
    rng = np.random.default_rng(seed + 77)
    anc = rng.integers(0, len(X), M)
    L = np.linalg.cholesky(cov)
    return X[anc] + 0.5 * rng.standard_normal((M, X.shape[1])) @ L.T, anc
