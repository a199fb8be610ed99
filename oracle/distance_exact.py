"""Exact references for the distance-and-accept chain: the p-norm distance
d = (sum_k |wf_k (x_k - x0_k)|^p)^(1/p) (max_k for p = inf) and the
UniformAcceptor decision d <= eps.

Test infrastructure only -- see ``oracle/__init__.py``.  Host only: numpy, the
standard library and mpmath.

``oracle.pnorm`` (float64 numpy) is a peer of the kernels: it rounds every
term, every partial sum and both powers.  Here every float64 input is the
rational it stands for (an integer times a power of two, as in
``oracle/weights_exact.py``); the difference, the product with the weight and,
for p in {1, 2, 3, inf}, the powers and their sum or max are Python integers.
The root (p = 2, 3) is taken by mpmath at ``digits`` (>= 40) and the result is
rounded ONCE to float64.  For any other p the powers, the sum and the root are
taken in mpmath at ``digits``: "exact" there means good to 10^-digits relative
(a half-integer p takes its per-term square roots from integers, to 10^-50:
mpmath's own pow costs 14 us per term, a minute over the device tests' inputs).

Special values -- the contract the kernels are held to, stated on the inputs
(not on what float64 arithmetic makes of them):

* a term is NaN when x_k, x0_k or wf_k is NaN, when x_k and x0_k are the same
  infinity (inf - inf), when wf_k = 0 meets an infinite x_k or x0_k (0 inf),
  or when an infinite wf_k meets x_k = x0_k (inf 0);
* otherwise a term is infinite when x_k, x0_k or wf_k is;
* a row with any NaN term is NaN, for every p (p = inf included: the max of a
  row that holds a NaN is NaN wherever the NaN sits); otherwise a row with any
  infinite term is +inf;
* -0.0 is 0: it is the rational 0.

A finite row whose exact distance lies past the largest double rounds to +inf
and one below the smallest subnormal to 0, as any single rounding does; what a
kernel makes of a finite row whose *intermediate* powers leave the float64
range is an edge of the format, not of this contract.
"""
import collections
import math

import numpy as np

from .weights_exact import EPS, U, ratio  # noqa: F401  (re-exported for the tests)

FINITE, INF, NAN = 0, 1, 2

PNormExact = collections.namedtuple("PNormExact", "d sum_p round_err kind")
PNormExact.__doc__ = """d [B] float64: the exact distance rounded once (NaN /
+inf per the special-value contract); sum_p [B] float64: sum_k |term_k|^p
(max_k |term_k| for p = inf) of the finite rows rounded once, NaN elsewhere;
round_err [B]: (d - exact) / exact of the finite rows with exact > 0 (what the
one rounding did, |.| <= u unless d is subnormal), 0 elsewhere; kind [B]:
FINITE, INF or NAN."""


def classify(x, x0, wf):
    """kind [B] of the rows of x [B, S] from the inputs alone."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    x0 = np.asarray(x0, dtype=np.float64)[None, :]
    wf = np.asarray(wf, dtype=np.float64)[None, :]
    xinf = np.isinf(x) | np.isinf(x0)
    nan_t = np.isnan(x) | np.isnan(x0) | np.isnan(wf)
    nan_t |= np.isinf(x) & np.isinf(x0) & (np.signbit(x) == np.signbit(x0))
    nan_t |= (wf == 0) & xinf
    nan_t |= np.isinf(wf) & ~xinf & (x == x0)
    inf_t = ~nan_t & (xinf | np.isinf(wf))
    kind = np.where(nan_t.any(1), NAN, np.where(inf_t.any(1), INF, FINITE))
    return kind.astype(np.int8)


def _ints(a):
    """float64 array (finite) -> (object array m of Python ints, int64 array e)
    with a == m 2^e exactly, element by element."""
    mant, ex = np.frexp(a)
    m53 = np.ldexp(mant, 53).astype(np.int64)          # exact: 53-bit integers
    return m53.astype(object), ex.astype(np.int64) - 53


def _term_ints(x, x0, wf):
    """|wf_k (x_bk - x0_k)| of finite inputs as integers T [B, S] (object) times
    2^g_k, one exponent per column."""
    B, S = x.shape
    mx, ex = _ints(x)
    m0, e0 = _ints(x0)
    mw, ew = _ints(wf)
    # one exponent per column for x and x0: the smallest in the column
    big = np.iinfo(np.int64).max
    exz = np.where(x != 0, ex, big)
    e0z = np.where(x0 != 0, e0, big)
    ec = np.minimum(exz.min(0) if B else np.full(S, big), e0z)
    ec = np.where(ec == big, 0, ec)
    shx = np.where(x != 0, ex - ec[None, :], 0).astype(object)
    sh0 = np.where(x0 != 0, e0 - ec, 0).astype(object)
    D = np.left_shift(mx, shx) - np.left_shift(m0, sh0)[None, :]
    T = np.abs(D * mw[None, :])
    return T, ec + ew


def _round_mpf(v):
    """An mpmath value rounded once to float64 (subnormals and overflow
    included)."""
    sign, man, ex, _ = v._mpf_
    return ratio(-int(man) if sign else int(man), 1, int(ex))


_isqrt = np.frompyfunc(math.isqrt, 1, 1)


def pnorm_exact(x, x0, wf, p, digits=50, half_integer_fast=True):
    """The exact p-norm distance of the rows of x [B, S] to x0 [S] under the
    weights wf [S] -> PNormExact.  p >= 1 or inf.  ``half_integer_fast``: take
    the square roots of a half-integer p (1.5, 2.5, ...) from integers instead
    of mpmath, to the same 10^-50 (digits <= 50 then)."""
    import mpmath
    assert digits >= 40 and (p >= 1)
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    x0 = np.asarray(x0, dtype=np.float64)
    wf = np.asarray(wf, dtype=np.float64)
    B, S = x.shape
    kind = classify(x, x0, wf)
    d = np.where(kind == NAN, np.nan, np.inf)
    sum_p = np.full(B, np.nan)
    rerr = np.zeros(B)
    fin = np.flatnonzero(kind == FINITE)
    if fin.size == 0:
        return PNormExact(d, sum_p, rerr, kind)
    # a finite row has finite x; a non-finite x0 or wf leaves no finite row
    T, g = _term_ints(x[fin], x0, wf)
    ctx = mpmath.mp.clone()
    ctx.dps = digits

    def finish(i, val, root):
        """val: mpf of sum_p; root: mpf of the distance."""
        d[i] = _round_mpf(root)
        sum_p[i] = _round_mpf(val)
        if root != 0 and d[i] != 0 and math.isfinite(d[i]):
            rerr[i] = float((ctx.mpf(float(d[i])) - root) / root)

    if p == math.inf or float(p) in (1.0, 2.0, 3.0):
        q = 1 if p == math.inf else int(p)
        gq = g * q
        G = int(gq.min())
        P = np.left_shift(T ** q, (gq - G).astype(object)[None, :])
        tot = P.max(1) if p == math.inf else P.sum(1)
        for i, v in zip(fin, tot.tolist()):
            # the integer to 10^-digits (exact below 2^(3.3 digits)); the
            # rounding to float64 of p = 1 and inf is taken from the integer
            val = ctx.ldexp(ctx.mpf(int(v)), G)
            if q == 1:
                d[i] = sum_p[i] = ratio(int(v), 1, G)
                if v and d[i] != 0 and math.isfinite(d[i]):
                    rerr[i] = float((ctx.mpf(float(d[i])) - val) / val)
            else:
                # a perfect power of fewer than 3.3 digits bits comes out exact
                finish(i, val, ctx.sqrt(val) if q == 2 else ctx.cbrt(val))
        return PNormExact(d, sum_p, rerr, kind)

    pm = ctx.mpf(float(p))
    inv = 1 / pm
    if half_integer_fast and float(2 * p).is_integer() and 2 * p < 64:
        # p = q / 2: t^q is an integer and its square root comes from
        # math.isqrt on >= 340 bits, i.e. to 2^-169 < 10^-50 relative -- the
        # precision mpmath works at below, without a Python-level pow per term
        # (14 us each; this path takes 1 us).  The root is mpmath's.
        q = int(2 * p)
        gq = g * q
        sh = 340 + (gq & 1)                       # gq - sh even
        R = _isqrt(np.left_shift(T ** q, sh.astype(object)[None, :]))
        h = (gq - sh) // 2
        H = int(h.min())
        tot = np.left_shift(R, (h - H).astype(object)[None, :]).sum(1)
        for i, v in zip(fin, tot.tolist()):
            s = ctx.ldexp(ctx.mpf(int(v)), H)
            finish(i, s, s ** inv if s != 0 else s)
        return PNormExact(d, sum_p, rerr, kind)
    Tl, gl = T.tolist(), [int(v) for v in g]
    for i, row in zip(fin, Tl):
        s = ctx.mpf(0)
        for t, gk in zip(row, gl):
            if t:
                s += ctx.ldexp(ctx.mpf(t), gk) ** pm
        finish(i, s, s ** inv if s != 0 else s)
    return PNormExact(d, sum_p, rerr, kind)


def accept_exact(d, eps):
    """The UniformAcceptor decision on float64 distances (the device's own):
    the ascending positions with d <= eps.  NaN is never accepted, by either
    side of the comparison, at eps = inf included."""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(d <= np.float64(eps))


def undecidable(ref, eps, rel_bound):
    """Rows whose exact distance lies within rel_bound x itself of eps: a
    kernel good to rel_bound may decide them either way.  ref: PNormExact;
    -> bool [B].  The exact distance is d / (1 + round_err); d - eps is exact
    in float64 wherever the two are within a factor of two (and the row is
    decidable where they are not).  NaN and infinite rows are decidable."""
    d = ref.d
    ok = (ref.kind == FINITE)
    with np.errstate(invalid="ignore", over="ignore"):
        exact_minus_eps = (d - eps) - d * ref.round_err
        out = ok & (np.abs(exact_minus_eps) <= rel_bound * d)
    return out


def accepted_exact(ref, eps):
    """bool [B]: the exact distance is <= eps (NaN rows never; infinite rows
    only at eps = inf)."""
    d = ref.d
    with np.errstate(invalid="ignore", over="ignore"):
        fin = (d - eps) - d * ref.round_err <= 0
        return np.where(ref.kind == FINITE, fin, (ref.kind == INF) & (eps == math.inf))
