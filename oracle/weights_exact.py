"""Exact references for the weight chain: importance weight, normalisation and
ESS, weighted moments, the cdf.

Test infrastructure only -- see ``oracle/__init__.py``.  Host only: numpy, the
standard library and (``importance_weight_exact``) mpmath.

numpy in float64 is a peer of the kernels, not a reference: its ``cumsum``
rounds N times, ``np.cov`` loses what the kernels lose.  Here every double is
an exact integer over a power-of-two denominator (``float.as_integer_ratio``,
vectorised through ``np.frexp``), sums and products are Python integers, and
each result is rounded ONCE, by Python's correctly rounded ``int / int``.  A
float64 result -- a kernel's or numpy's -- can then be measured.

A weighted covariance needs no centring in exact arithmetic:
    sum w (x_a - m_a)(x_b - m_b) / sum w = (S Q_ab - P_a P_b) / S^2,
    S = sum w,  P = sum w x,  Q = sum w x x^T
which are all integers.  ``exact_moments`` does this while N d^2 is small
(``EXACT_LIMIT``); beyond it the same three sums run in vectorised
double-double arithmetic whose own error is stated at ``_dd_moments``.
"""
import collections
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)      # 2^-52
U = EPS / 2                                # unit roundoff
TINY = 5e-324                              # spacing of the subnormals
EXACT_LIMIT = 6_000_000                    # N d (d + 1) / 2 integer products


# ---- doubles as integers ------------------------------------------------------

def to_ints(a):
    """float64 array (finite) -> (object array of Python ints m, e) with
    a == m * 2^e exactly, one exponent for the whole array."""
    a = np.asarray(a, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError("to_ints: non-finite input")
    mant, ex = np.frexp(a)                         # a = mant 2^ex, |mant| < 1
    m53 = np.ldexp(mant, 53).astype(np.int64)      # exact: 53-bit integers
    ex = ex.astype(np.int64) - 53
    nz = m53 != 0
    e = int(ex[nz].min()) if nz.any() else 0
    sh = np.where(nz, ex - e, 0)
    out = np.empty(a.shape, dtype=object)
    flat_o, flat_m, flat_s = out.reshape(-1), m53.reshape(-1), sh.reshape(-1)
    for i in range(flat_o.size):
        flat_o[i] = int(flat_m[i]) << int(flat_s[i])
    return out, e


def ratio(num, den, e=0):
    """num / den * 2^e for Python ints, rounded once to float64 (subnormal
    results included; +-inf on overflow; NaN for 0 / 0)."""
    num, den = int(num), int(den)
    if den == 0:
        return math.nan if num == 0 else (math.inf if num > 0 else -math.inf)
    if e >= 0:
        num <<= e
    else:
        den <<= -e
    try:
        return num / den
    except OverflowError:
        return math.inf if (num > 0) == (den > 0) else -math.inf


# ---- sums, normalised weights, ESS ---------------------------------------------

Sums = collections.namedtuple("Sums", "sum sum_sq max ess normalised ints e")
Sums.__doc__ = """sum, sum_sq, max, ess: float64, each rounded once from its
exact value (ess = (sum w)^2 / sum w^2 as one rational: it is the same for w
and for c w); normalised: the correctly rounded w / sum w; ints, e: w as
integers times 2^e."""


def exact_sums(w):
    m, e = to_ints(w)
    S = sum(m.tolist())
    S2 = sum(v * v for v in m.tolist())
    wn = np.array([ratio(v, S) for v in m.tolist()], dtype=np.float64)
    return Sums(ratio(S, 1, e), ratio(S2, 1, 2 * e),
                float(np.max(w)) if len(m) else math.nan,
                ratio(S * S, S2), wn, m, e)


# ---- cdf --------------------------------------------------------------------------

Prefix = collections.namedtuple("Prefix", "ints e values")
Prefix.__doc__ = """ints[i] 2^e = w_0 + .. + w_i exactly; values: their
correctly rounded float64."""


def exact_prefix(w):
    m, e = to_ints(w)
    acc, run = [], 0
    for v in m.tolist():
        run += v
        acc.append(run)
    vals = np.array([ratio(v, 1, e) for v in acc], dtype=np.float64)
    return Prefix(acc, e, vals)


# ---- moments ----------------------------------------------------------------------

Moments = collections.namedtuple(
    "Moments", "sum sum_sq max mean cov A M own_error")
Moments.__doc__ = """sum w, sum w^2, max w, the weighted mean [d] and
cov = sum w (x-m)(x-m)^T / sum w [d, d], each entry rounded once from its
exact value (own_error = 0) or from double-double sums (own_error: a bound on
|cov - exact| / A and |mean - exact| / M, see ``_dd_moments``);
A_ab = sum w |x_a-m_a| |x_b-m_b| / sum w and M_a = sum w |x_a| / sum w: the
magnitudes a rounding-error bound is stated in (float64; they only scale a
bound)."""


def _magnitudes(X, w, mean):
    sw = w.sum()
    M = (w[:, None] * np.abs(X)).sum(0) / sw
    C = np.abs(X - mean)
    A = (w[:, None] * C).T @ C / sw
    return A, M


def exact_moments(X, w, force_exact=False):
    X = np.asarray(X, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    N, d = X.shape
    if not force_exact and N * d * (d + 1) // 2 > EXACT_LIMIT:
        return _dd_moments(X, w)
    wm, ew = to_ints(w)
    S = sum(wm.tolist())
    S2 = sum(v * v for v in wm.tolist())
    cols = [to_ints(X[:, a]) for a in range(d)]      # one exponent per column
    xm = np.empty((N, d), dtype=object)
    for a in range(d):
        xm[:, a] = cols[a][0]
    ex = [c[1] for c in cols]
    wx = xm * wm[:, None]                            # w x, units 2^(ew + ex_a)
    P = wx.sum(0)
    mean = np.array([ratio(P[a], S, ex[a]) for a in range(d)])
    cov = np.empty((d, d))
    for a in range(d):
        # Q_ab for b >= a in one object dot
        Q = wx[:, a] @ xm[:, a:]
        Q = np.atleast_1d(Q)
        for k, b in enumerate(range(a, d)):
            cov[a, b] = cov[b, a] = ratio(S * Q[k] - P[a] * P[b], S * S,
                                          ex[a] + ex[b])
    A, M = _magnitudes(X, w, mean)
    return Moments(ratio(S, 1, ew), ratio(S2, 1, 2 * ew), float(w.max()),
                   mean, cov, A, M, 0.0)


# double-double: a value is hi + lo with |lo| <= ulp(hi) / 2.  two_sum is
# Knuth's, two_prod Dekker's with Veltkamp's split (numpy has no fma); both are
# error-free unless a product over- or underflows.
_SPLIT = 134217729.0     # 2^27 + 1


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    t = _SPLIT * a
    hi = t - (t - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_add(ah, al, bh, bl):
    s, e = _two_sum(ah, bh)
    e = e + (al + bl)
    return _two_sum(s, e)


def _dd_mul_d(ah, al, b):
    p, e = _two_prod(ah, b)
    e = e + al * b
    return _two_sum(p, e)


def _dd_sum0(h, l):
    """Pairwise sum over axis 0 of double-double arrays."""
    while h.shape[0] > 1:
        if h.shape[0] & 1:
            z = np.zeros((1,) + h.shape[1:])
            h, l = np.concatenate([h, z]), np.concatenate([l, z])
        h, l = _dd_add(h[0::2], l[0::2], h[1::2], l[1::2])
    return h[0], l[0]


def _dd_moments(X, w):
    """Two-pass moments in double-double: the mean as a double-double, rows
    centred on it in double-double, products and pairwise sums in
    double-double.  Every operation is good to 2^-104 relative (4 u^2); a term
    w (x_a - m_a)(x_b - m_b) meets 4 of them and log2 N + 1 additions, the
    centring on an inexact mean adds the square of the mean's error, so
    |cov_ab - exact| <= (6 + log2 N) 4 u^2 A_ab + (..)^2 M_a M_b and likewise
    for the mean with M_a: ``own_error`` = (6 + log2 N) 4 u^2 + 2 u (the final
    division and rounding in float64), ~2.3e-16 -- against kernel bounds of 1e-14 and
    more.  Inputs are scaled per column by a power of two first so that no
    product under- or overflows."""
    N, d = X.shape
    cs = np.ones(d)
    for a in range(d):
        mx = np.abs(X[:, a]).max()
        if mx > 0:
            cs[a] = 2.0 ** -math.frexp(mx)[1]
    Xs = X * cs                                   # exact
    ws = w * 2.0 ** -math.frexp(w.max())[1] if w.max() > 0 else w
    Sh, Sl = _dd_sum0(ws.copy(), np.zeros(N))
    ph, pl = _two_prod(ws[:, None], Xs)
    Ph, Pl = _dd_sum0(ph, pl)
    # mean = P / S in double-double (one Newton step on the float64 quotient)
    q = Ph / Sh
    rh, rl = _dd_mul_d(np.full(d, Sh), np.full(d, Sl), q)
    dh, dl = _dd_add(Ph, Pl, -rh, -rl)
    mh, ml = _two_sum(q, (dh + dl) / Sh)
    ch, cl = _dd_add(Xs, np.zeros_like(Xs), -mh[None, :], -ml[None, :])
    cov = np.empty((d, d))
    for a in range(d):
        # w c_a (double-double) times c_b (double-double), b >= a
        th, tl = _dd_mul_d(ch[:, a], cl[:, a], ws)
        uh, ul = _two_prod(th[:, None], ch[:, a:])
        ul = ul + (th[:, None] * cl[:, a:] + tl[:, None] * ch[:, a:])
        uh, ul = _two_sum(uh, ul)
        Qh, Ql = _dd_sum0(uh, ul)
        cov[a, a:] = (Qh / Sh + (Ql - (Qh / Sh) * Sl) / Sh) / (cs[a] * cs[a:])
        cov[a:, a] = cov[a, a:]
    mean = (mh + ml) / cs
    A, M = _magnitudes(X, w, mean)
    own = (6 + math.log2(max(N, 2))) * 4 * U * U + 2 * U
    return Moments(float(np.sum(w)), float(np.sum(w * w)), float(w.max()),
                   mean, cov, A, M, own)


# ---- importance weight ----------------------------------------------------------------

def importance_weight_exact(lp, lt, scale, accw=None, digits=50):
    """exp(lp - lt) * scale * accw with the difference exact, the exponential
    in mpmath at ``digits`` (>= 40) and ONE rounding to float64 (gradual
    underflow and overflow to inf included).  Non-finite inputs follow IEEE:
    lp = -inf -> 0, lt = -inf -> +inf (scale > 0), NaN anywhere -> NaN."""
    import mpmath
    assert digits >= 40
    lp = np.atleast_1d(np.asarray(lp, dtype=np.float64))
    lt = np.atleast_1d(np.asarray(lt, dtype=np.float64))
    aw = None if accw is None else np.atleast_1d(np.asarray(accw, dtype=np.float64))
    out = np.empty(len(lp))
    ctx = mpmath.mp.clone()
    ctx.dps = digits
    for i in range(len(lp)):
        a, b = float(lp[i]), float(lt[i])
        c = 1.0 if aw is None else float(aw[i])
        if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)
                and math.isfinite(scale)):
            with np.errstate(all="ignore"):
                v = np.exp(np.float64(a) - np.float64(b)) * np.float64(scale)
                out[i] = v * c if aw is not None else v
            continue
        v = ctx.exp(ctx.mpf(a) - ctx.mpf(b)) * ctx.mpf(scale) * ctx.mpf(c)
        sign, man, ex, _ = v._mpf_
        num = -int(man) if sign else int(man)
        out[i] = ratio(num, 1, int(ex))
    return out
