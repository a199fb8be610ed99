"""Extended-precision LocalTransition reference and ill-conditioned populations.

Test infrastructure only -- see ``oracle/__init__.py``.

``oracle.local_fit`` / ``oracle.local_logpdf`` are float64: on a ridge with
condition number kappa their own error is ~eps * kappa in the thin direction,
the same order as the kernels'.  The functions here evaluate the same
definitions beyond float64 -- the fit from exact integer sums and mpmath at 40
digits, the density in 80-bit ``np.longdouble`` where it has a 64-bit mantissa
(else mpmath) -- so that a float64 result, the oracle's or a kernel's, can be
measured, not just compared with a peer.

Errors are measured in the metric of the exact covariance (``whitened``): the
relative error of the Mahalanobis form x^T A x over all x, which is what the
density sees.  An entrywise rtol on ``covs`` says nothing about the thin
direction.
"""
import numpy as np

EPS64 = np.finfo(np.float64).eps
LONGDOUBLE_OK = np.finfo(np.longdouble).eps < 2e-19


class _LongDouble:
    name = "longdouble"

    @staticmethod
    def arr(a):
        return np.asarray(a, dtype=np.longdouble)

    log = staticmethod(np.log)
    exp = staticmethod(np.exp)
    sqrt = staticmethod(np.sqrt)

    @staticmethod
    def zeros(shape):
        return np.zeros(shape, dtype=np.longdouble)


class _MpMath:
    """Object arrays of mpmath.mpf at 40 digits (slow: small cases only)."""
    name = "mpmath"

    def __init__(self):
        import mpmath
        self.mp = mpmath.mp.clone()
        self.mp.dps = 40
        self._log = np.frompyfunc(self.mp.log, 1, 1)
        self._exp = np.frompyfunc(self.mp.exp, 1, 1)
        self._sqrt = np.frompyfunc(self.mp.sqrt, 1, 1)
        self._mpf = np.frompyfunc(lambda v: self.mp.mpf(float(v))
                                  if isinstance(v, (float, int, np.floating, np.integer))
                                  else self.mp.mpf(v), 1, 1)

    def arr(self, a):
        a = np.asarray(a)
        if a.dtype == object:
            return a
        hi = a.astype(np.float64)
        if a.dtype != np.longdouble:
            return self._mpf(hi)
        # a longdouble is the exact sum of two float64
        return self._mpf(hi) + self._mpf((a - hi).astype(np.float64))

    def log(self, a):
        return self._log(a)

    def exp(self, a):
        return self._exp(a)

    def sqrt(self, a):
        return self._sqrt(a)

    def zeros(self, shape):
        out = np.empty(shape, dtype=object)
        out[...] = self.mp.mpf(0)
        return out


def backend(name=None):
    """``"longdouble"``, ``"mpmath"`` or None (longdouble where it is 80-bit)."""
    if name is None:
        name = "longdouble" if LONGDOUBLE_OK else "mpmath"
    return _LongDouble() if name == "longdouble" else _MpMath()


def f64(a):
    """Round an extended-precision array to float64."""
    a = np.asarray(a)
    if a.dtype == object:
        return np.vectorize(float, otypes=[np.float64])(a)
    return a.astype(np.float64)


# ---- small dense linear algebra that works on longdouble and object arrays --

def _cholesky(xp, C):
    d = C.shape[0]
    L = xp.zeros((d, d))
    for a in range(d):
        for b in range(a + 1):
            s = C[a, b] - (L[a, :b] * L[b, :b]).sum() if b else C[a, b]
            if a == b:
                if not s > 0:
                    raise np.linalg.LinAlgError("exact covariance not positive definite")
                L[a, a] = xp.sqrt(s)
            else:
                L[a, b] = s / L[b, b]
    return L


def _lower_inverse(xp, L):
    d = L.shape[0]
    Li = xp.zeros((d, d))
    for c in range(d):
        Li[c, c] = 1 / L[c, c]
        for a in range(c + 1, d):
            Li[a, c] = -(L[a, c:a] * Li[c:a, c]).sum() / L[a, a]
    return Li


def neighbours(X, i, k):
    """The k neighbours of particle i as ``oracle.local_fit`` takes them:
    float64 squared distances, (distance, index) order, the first (self)
    dropped.  Also returns the sorted squared distances."""
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    nq = min(k + 1, n)
    d2 = ((X - X[i]) ** 2).sum(1)
    order = np.lexsort((np.arange(n), d2))
    return order[1:nq], d2[order]


def _exact_ints(a):
    """float64 array -> (object array of Python ints m, exponent e) with
    a == m * 2^e exactly."""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)
    m53 = (m * 2.0 ** 53).astype(np.int64)        # exact: 53-bit mantissas
    e = e.astype(np.int64) - 53
    emin = int(e[m53 != 0].min()) if (m53 != 0).any() else 0
    sh = np.where(m53 != 0, e - emin, 0)
    ints = np.array([int(v) << int(s) for v, s in zip(m53.ravel(), sh.ravel())],
                    dtype=object).reshape(a.shape)
    return ints, emin


def _two_pass_cov(D, wn):
    """np.cov(aweights) of offsets D [k, d] with neighbour weights wn [k]."""
    a = wn / wn.sum()
    E = D - (a[:, None] * D).sum(0)
    return ((a[:, None] * E).T[:, None, :] * E.T[None, :, :]).sum(2) / (1 - (a * a).sum())


def exact_local_fit(X, w, k, rows, method="exact"):
    """Local fit (scaling = 1) of the given rows beyond float64.

    C* = sum a (d - dbar)(d - dbar)^T / (1 - sum a^2), a = w / sum w over the
    neighbours (``np.cov(aweights)`` semantics), A* = C*^-1 and log det C* from
    its Cholesky factor.  method:

    - ``"exact"``: the float64 inputs are integers times a power of two, so
      the raw sums S0 = sum w, S1 = sum w d, S2 = sum w d d^T, Q = sum w^2 are
      summed exactly in Python integers and C* = (S0 S2 - S1 S1^T) / (S0^2 - Q)
      is one exact ratio per entry (no cancellation to round); only the d x d
      factorisations round, in mpmath at 40 digits.
    - ``"mpmath"``: the two-pass form, every step at 40 digits (an independent
      statement of the same definition).
    - ``"longdouble"``: the two-pass form in 80-bit longdouble.  Fast, but C*
      rounded entrywise to a 64-bit mantissa is already 2^-64 cond(C*) out in
      the whitened metric (5e-12 at cond 1e8): enough to supply a density test
      with a fit, not to measure a float64 fit at cond 1e8 against 1e-17.

    Returns arrays of the method's number type: ``C`` [R, d, d], ``A``, ``L``,
    ``Linv``, ``logdet`` [R]; the neighbour indices ``nb``; the relative gap
    between the k-th and (k+1)-th squared distances ``gap`` (inf when every
    other particle is a neighbour); and the backend ``xp``.
    """
    xp = backend("longdouble" if method == "longdouble" else "mpmath")
    X64 = np.asarray(X, dtype=np.float64)
    w64 = np.asarray(w, dtype=np.float64)
    n, d = X64.shape
    if method == "exact":
        Xe, ex = _exact_ints(X64)
        we, _ = _exact_ints(w64)
    else:
        Xe, we = xp.arr(X64), xp.arr(w64)
    rows = np.asarray(rows)
    R = len(rows)
    out = dict(C=xp.zeros((R, d, d)), A=xp.zeros((R, d, d)), L=xp.zeros((R, d, d)),
               Linv=xp.zeros((R, d, d)), LT=xp.zeros((R, d, d)), logdet=xp.zeros(R), nb=[],
               gap=np.empty(R),
               rows=rows, k=k, xp=xp)
    for o, i in enumerate(rows):
        nb, d2s = neighbours(X64, int(i), k)
        kk = len(nb)
        out["gap"][o] = ((d2s[kk + 1] - d2s[kk]) / d2s[kk + 1]) if kk + 1 < n else np.inf
        D = Xe[nb] - Xe[int(i)]
        if method == "exact":
            wn = we[nb]
            wD = wn[:, None] * D
            S0, S1, Q = wn.sum(), wD.sum(0), (wn * wn).sum()
            S2 = (wD.T[:, None, :] * D.T[None, :, :]).sum(2)
            num = S0 * S2 - S1[:, None] * S1[None, :]
            mpf = xp.mp.mpf
            scale = mpf(2) ** (2 * ex) / mpf(S0 * S0 - Q)
            C = np.array([[mpf(int(v)) * scale for v in r] for r in num], dtype=object)
        else:
            C = _two_pass_cov(D, we[nb])
        L = _cholesky(xp, C)
        Li = _lower_inverse(xp, L)
        out["C"][o] = C
        out["L"][o] = L
        out["Linv"][o] = Li
        out["LT"][o] = L.T
        for a in range(d):          # A* = Linv^T Linv (Linv lower triangular)
            for b in range(a + 1):
                out["A"][o][a, b] = out["A"][o][b, a] = (Li[a:, a] * Li[a:, b]).sum()
        out["logdet"][o] = 2 * xp.log(np.diagonal(L)).sum()
        out["nb"].append(nb)
    return out


def _ld(a):
    """Extended-precision array -> longdouble (an mpf as the sum of two
    float64: 106 bits kept, more than the 64 a longdouble holds)."""
    a = np.asarray(a)
    if a.dtype != object:
        return a.astype(np.longdouble)
    hi = f64(a)
    return hi.astype(np.longdouble) + f64(a - hi).astype(np.longdouble)


def _whiten(fit, key, o, delta):
    # The difference from the exact matrix is taken in the fit's precision
    # (that is the cancellation); the congruence then runs in longdouble: it
    # multiplies an error matrix, whose own relative accuracy need not be high
    # (terms of size cond |delta| cancel to the result: 2^-64 cond relative).
    T = _ld(fit[key][o])
    return float(np.linalg.norm(f64(T @ _ld(delta) @ T.T), 2))


def whitened(C, fit, o):
    """||L*^-1 (C - C*) L*^-T||_2 for row o of an ``exact_local_fit``."""
    return _whiten(fit, "Linv", o, fit["xp"].arr(np.asarray(C)) - fit["C"][o])


def whitened_inv(A, fit, o):
    """||L*^T A L* - I||_2 = ||L*^T (A - A*) L*||_2 for row o of an
    ``exact_local_fit``."""
    return _whiten(fit, "LT", o, fit["xp"].arr(np.asarray(A)) - fit["A"][o])


def exact_local_logpdf(x, X, w, inv_covs, log_norm, xp=None, with_q=False):
    """log( sum_j w_j exp(-d_ij^T A_j d_ij / 2 - log_norm_j) / sum_j w_j ),
    d_ij = X_j - x_i, with direct differences and a log-sum-exp in extended
    precision.  The float64 ``inv_covs`` / ``log_norm`` are exact inputs: this
    is the function of them that abc_local_logpdf computes.  Returns float64
    (-inf only when every weight is zero).  with_q: also the largest q_ij of
    each candidate among the terms within 2^-53 of its largest (the pairs that
    take part in a float64 result)."""
    xp = xp or backend()
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    X = np.asarray(X, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    keep = w > 0
    # (an extended-precision fit may be passed as it is: the composed test)
    Xe, A = xp.arr(X[keep]), xp.arr(np.asarray(inv_covs)[keep])
    c = xp.log(xp.arr(w[keep])) - xp.arr(np.asarray(log_norm)[keep])
    logW = xp.log(xp.arr(w).sum())
    out = np.empty(len(x))
    qmax = np.zeros(len(x))
    for i in range(len(x)):
        D = Xe - xp.arr(x[i])
        q = ((D[:, :, None] * A).sum(1) * D).sum(1)
        t = c - q / 2
        m = t.max()
        s = xp.exp(t - m)
        out[i] = float(m + xp.log(s.sum()) - logW)
        if with_q:
            qmax[i] = float(q[f64(t - m) >= -53 * np.log(2)].max())
    return (out, qmax) if with_q else out


# ---- populations -------------------------------------------------------------

def ridge_population(N, d, kappa, sep, seed, stray=None, scale=1.0, stray_row=0):
    """A rotated ridge: standard normals scaled by (1, .., 1, kappa^-1/2)
    (times ``scale``), rotated by a random orthogonal Q, offset by +7; for
    sep > 0 rows N/2.. are moved sep * Q[:, 0] (a second mode along a wide
    direction); ``stray = s`` sets X[stray_row] = s in every coordinate.
    Weights exp(0.3 * normal), normalised.  Returns X, w, Q."""
    rng = np.random.default_rng(seed)
    s = np.ones(d)
    s[-1] = kappa ** -0.5
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    X = (rng.standard_normal((N, d)) * (scale * s)) @ Q.T + 7.0
    if sep > 0:
        X[N // 2:] += sep * Q[:, 0]
    if stray is not None:
        X[stray_row] = stray
    w = np.exp(0.3 * rng.standard_normal(N))
    w /= w.sum()
    return X, w, Q


def check_rows(X, Q, seed, n=16):
    """The rows a fit test checks: row 0, row N-1, two rows of each mode, the
    rows with the extreme projections on Q[:, 0] and Q[:, -1] (boundary
    particles: their neighbour offsets have the largest mean), filled up to n
    with random rows."""
    N = len(X)
    rows = [0, N - 1, N // 7, N // 3, N // 2 + 5, N - N // 5]
    for a in (0, -1):
        p = X @ Q[:, a]
        rows += [int(p.argmin()), int(p.argmax())]
    rng = np.random.default_rng(seed + 1)
    for r in rng.permutation(N):
        if len(set(rows)) >= n:
            break
        rows.append(int(r))
    return np.array(sorted(set(rows)))


# ---- the cases of tests/test_gpu_local_conditioning.py ----------------------
# (shared with tests/test_oracle_local_exact.py, which asserts the conditions
# on these inputs without a GPU)

# N, d, k: the smallest shapes that reach each moments route of launch_fit
FIT_SHAPES = {
    "radix+valu": [(600, 3, 20)],
    "dense-mm": [(1500, 3, 400), (1000, 5, 260), (1500, 2, 400)],
    "knn-list": [(2500, 5, 50), (2500, 8, 90)],
    "knn+valu": [(3000, 5, 170)],
    "knn+dense-defer": [(3000, 3, 700), (4096, 2, 1024)],
    "sliced": [(2500, 12, 100), (2100, 16, 300)],
    "wide-control": [(400, 20, 40)],
}
DENSE_ROUTES = ("dense-mm", "knn+dense-defer")
# kappa, sep, stray
FIT_POPULATIONS = [(1e4, 0, None), (1e6, 0, None), (1e6, 30, None), (1e8, 0, None),
                   (1e8, 30, None)]
FIT_POPULATIONS_DENSE = [(1e4, 0, 1e4), (1e6, 0, 30.0)]


def fit_cases():
    """(route, N, d, k, kappa, sep, stray) of every fit case."""
    out = []
    for route, shapes in FIT_SHAPES.items():
        for (N, d, k) in shapes:
            pops = FIT_POPULATIONS + (FIT_POPULATIONS_DENSE if route in DENSE_ROUTES else [])
            for (kappa, sep, stray) in pops:
                out.append((route, N, d, k, kappa, sep, stray))
    return out


def fit_case_inputs(N, d, k, kappa, sep, stray):
    seed = int(N + 31 * d + k + np.log10(kappa) * 7 + sep)
    X, w, Q = ridge_population(N, d, kappa, sep, seed, stray=stray)
    return X, w, Q, check_rows(X, Q, seed)


# d, N, M
PDF_SHAPES = [(2, 601, 130), (5, 601, 130), (8, 601, 70), (12, 333, 65), (16, 333, 65)]
# kappa, sep, scale, stray, stray_row (-1: the last row)
PDF_POPULATIONS = ([(1e4, 0, 1.0, None, 0), (1e6, 30, 1.0, None, 0),
                    (1e6, 300, 1.0, None, 0), (1e8, 30, 1.0, None, 0)] +
                   [(1.0, 0, 0.3, s, r) for r in (0, -1) for s in (1e3, 1e4, 1e5)])


def pdf_cases():
    return [(d, N, M) + pop for (d, N, M) in PDF_SHAPES for pop in PDF_POPULATIONS]


def pdf_case_inputs(d, N, M, kappa, sep, scale, stray, stray_row):
    """Population, exact fit of every row rounded to float64, candidates: a
    population row plus 0.3 local standard deviations in that row's own
    metric (its exact Cholesky factor); candidate 0 is moved 1e4 away."""
    seed = int(1000 * d + N + np.log10(kappa) * 7 + sep + (0 if stray is None else np.log10(stray)))
    X, w, Q = ridge_population(N, d, kappa, sep, seed, stray=stray, scale=scale,
                               stray_row=stray_row % N)
    k = max(N // 4, 10, d)
    # (the density takes this fit as an exact input: longdouble accuracy is
    # ample, and all N rows at 40 digits would take minutes)
    fit = exact_local_fit(X, w, k, np.arange(N), method="longdouble" if LONGDOUBLE_OK else "exact")
    inv, L = f64(fit["A"]), f64(fit["L"])
    lnorm = 0.5 * (d * np.log(2 * np.pi) + f64(fit["logdet"]))
    rng = np.random.default_rng(seed + 2)
    r = rng.integers(0, N, M)
    r[1] = stray_row % N          # a candidate beside the stray / an end row
    x = X[r] + 0.3 * np.einsum("mab,mb->ma", L[r], rng.standard_normal((M, d)))
    x[0] += 1e4
    return dict(X=X, w=w, inv=inv, lnorm=lnorm, x=x, fit=fit, k=k)
