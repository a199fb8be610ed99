"""numpy replay of the integer-parameter kernels (pyabc_amd/csrc/abc_walk.hip):
grid-prior draws and log mass, random-walk proposals with the prior re-draw
loop, and the walk's mass in exact rational arithmetic.  Built on the
oracle's Philox and uniform helpers; test code only."""
from fractions import Fraction

import numpy as np

from oracle.philox import philox4x32_10, uniform53
from oracle.sampler import (SLOT_PERTURB, SLOTS_PER_ATTEMPT, prior_uniforms)


def last_positive(a):
    return int(np.nonzero(np.asarray(a) > 0)[0][-1])


# ---- grid prior: spec = [(k_lo, pmf, logpmf)] per coordinate ----------------

def grid_draw(spec, seed, generation, idx0, B):
    """abc_grid_prior_draw: theta [B, d]."""
    idx = (np.uint64(idx0) + np.arange(B, dtype=np.uint64))
    theta = np.empty((B, len(spec)))
    for k, (k_lo, pmf, _) in enumerate(spec):
        cdf = np.cumsum(np.asarray(pmf, dtype=np.float64))
        u = prior_uniforms(idx, np.ones(B, dtype=np.int64), k, generation, seed)
        i = np.searchsorted(cdf, u * cdf[-1], side="left")   # first cdf >= t
        theta[:, k] = k_lo + np.minimum(i, last_positive(pmf))
    return theta


def grid_logpmf(theta, spec):
    """abc_grid_prior_logpmf: the terms summed in ascending k; -inf outside a
    window, NaN for a value that is no integer."""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    lp = np.zeros(len(theta))
    with np.errstate(invalid="ignore"):
        for k, (k_lo, pmf, logpmf) in enumerate(spec):
            v = theta[:, k]
            term = np.full(len(v), np.nan)
            whole = v == np.floor(v)
            out = whole & ((v < k_lo) | (v > k_lo + len(pmf) - 1))
            term[out] = -np.inf
            ins = whole & ~out
            term[ins] = np.asarray(logpmf)[(v[ins] - k_lo).astype(np.int64)]
            lp = lp + term
    return lp


# ---- the walk ------------------------------------------------------------------

def exact_step_law(n, p_l, p_r, p_c):
    """The law of the sum of n steps in {-1, 0, +1}: n-fold convolution of
    the one-step law in rational arithmetic (index s + n)."""
    one = [Fraction(p_l), Fraction(p_c), Fraction(p_r)]
    law = [Fraction(1)]
    for _ in range(n):
        new = [Fraction(0)] * (len(law) + 2)
        for i, a in enumerate(law):
            for j, b in enumerate(one):
                new[i + j] += a * b
        law = new
    return law


def displacement_index(u, cum, last):
    """The law's index drawn by the uniform u in [0, 1): first index with
    cum > u cum[-1], at most `last` (the last index of positive law)."""
    i = np.searchsorted(cum, np.asarray(u) * cum[-1], side="right")
    return np.minimum(i, last)


def walk_propose(X, w, law, seed, generation, idx0, B, spec=None, max_attempts=1):
    """abc_walk_propose: (theta, prior log mass, ancestor, attempts).  X
    integer-valued [N, d]; law [2 n + 1]; spec: a grid prior or None (plain
    rvs: one attempt, log mass 0)."""
    X = np.asarray(X, dtype=np.int64)
    N, d = X.shape
    law = np.asarray(law, dtype=np.float64)
    n = (len(law) - 1) // 2
    cum, last = np.cumsum(law), last_positive(law)
    cdf = np.cumsum(np.asarray(w, dtype=np.float64))
    total = cdf[-1]
    if spec is None:
        max_attempts = 1
    idx = (np.uint64(idx0) + np.arange(B, dtype=np.uint64))
    theta = np.empty((B, d))
    lp = np.full(B, -np.inf)
    anc = np.empty(B, dtype=np.int64)
    att = np.full(B, max_attempts + 1, dtype=np.int64)
    todo = np.ones(B, dtype=bool)
    for a in range(max_attempts):
        pos = np.nonzero(todo)[0]
        if len(pos) == 0:
            break
        ii = idx[pos]
        s0 = a * SLOTS_PER_ATTEMPT
        r = philox4x32_10(ii, s0, generation, seed)
        j = np.minimum(np.searchsorted(cdf, uniform53(r[:, 0], r[:, 1]) * total,
                                       side="right"), N - 1)
        th = np.empty((len(pos), d))
        for k in range(d):
            if k % 2 == 0:
                r = philox4x32_10(ii, s0 + SLOT_PERTURB + k // 2, generation, seed)
            u = uniform53(r[:, 2 * (k & 1)], r[:, 2 * (k & 1) + 1])
            th[:, k] = X[j, k] + displacement_index(u, cum, last) - n
        l = np.zeros(len(pos)) if spec is None else grid_logpmf(th, spec)
        theta[pos], anc[pos] = th, j
        ok = l > -np.inf
        lp[pos[ok]] = l[ok]
        att[pos[ok]] = a + 1
        todo[pos[ok]] = False
    return theta, lp, anc, att


def exact_mass(x, X, w, law):
    """sum_j w_j prod_k law[x_ik - X_jk + n] per row of x, the float64 table
    entries and weights taken as rationals: a list of Fractions."""
    import math

    def split(v):                    # v = m 2^e exactly, m an integer
        m, e = math.frexp(float(v))
        return int(m * 2 ** 53), e - 53

    X = np.asarray(X, dtype=np.int64)
    n = (len(law) - 1) // 2
    fl = [split(v) for v in law]
    fw = [split(v) for v in w]
    out = []
    for row in np.atleast_2d(x):
        row = np.asarray(row, dtype=np.int64)
        s = row[None, :] - X
        near = np.nonzero((np.abs(s) <= n).all(axis=1))[0]
        terms = []
        for j in near:
            m, e = fw[j]
            for k in range(X.shape[1]):
                lm, le = fl[int(s[j, k]) + n]
                m, e = m * lm, e + le
            if m:
                terms.append((m, e))
        if not terms:
            out.append(Fraction(0))
            continue
        e0 = min(e for _, e in terms)
        tot = sum(m << (e - e0) for m, e in terms)
        out.append(Fraction(tot) * Fraction(2) ** e0)
    return out


def log_fraction(f):
    """log of a non-negative Fraction, correctly rounded where mpmath is
    installed (-inf for 0); else log of the correctly rounded double, which
    is within 2^-53 (1 + |log f| / 2) of it for f in the double range."""
    import math
    if f == 0:
        return -math.inf
    try:
        import mpmath
    except ImportError:
        return math.log(float(f))
    with mpmath.workprec(200):
        return float(mpmath.log(mpmath.mpf(f.numerator) / mpmath.mpf(f.denominator)))
