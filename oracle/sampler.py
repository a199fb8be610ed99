"""Replay of the batched sampler's counter-based draws in numpy (float64).

Test infrastructure only -- see ``oracle/__init__.py``.  The semantics are
those of pyabc/smc.py:610-662 (_generate_valid_proposal: theta =
Transition.rvs(), re-draw while the prior density is 0) and
pyabc/transition/multivariatenormal.py:85-97 (ancestor ~ Cat(w) by inverse
CDF, theta = X_j + N(0, Sigma)); only the random stream differs from the
reference (numpy MT19937 there, Philox keyed by the global candidate index
here), so the device and this replay agree draw for draw.
"""
import numpy as np
from scipy import stats

from .philox import philox4x32_10, uniform01, uniform53, normal_pairs

SLOTS_PER_ATTEMPT = 65536
SLOT_PERTURB = 1
SLOT_PRIOR = 32
SLOT_SIM = 0x40000000

KIND = {"flat": -1, "norm": 0, "uniform": 1, "expon": 2, "laplace": 3,
        "lognorm": 4, "gamma": 5, "beta": 6}


def normals(index, slot0, n, generation, seed):
    """n normals per candidate: normal q from slot slot0 + q // 4."""
    index = np.asarray(index, dtype=np.uint64)
    out = np.empty((len(index), n))
    for q in range(0, n, 4):
        r = philox4x32_10(index, slot0 + q // 4, generation, seed)
        a0, a1 = normal_pairs(r[:, 0], r[:, 1])
        b0, b1 = normal_pairs(r[:, 2], r[:, 3])
        block = np.stack([a0, a1, b0, b1], axis=1)
        out[:, q:q + 4] = block[:, :min(4, n - q)]
    return out


def perturbation_normals(index, slot0, n, generation, seed, anc_words):
    """The n perturbation normals of one attempt (pyabc_amd/csrc/
    abc_candidate.h perturb_words): normals 0, 1 from the ancestor draw's
    unused words 2, 3 (anc_words [B, 4]); normals 2 q' + 2, 2 q' + 3 from half
    q' & 1 of slot slot0 + q' // 2."""
    index = np.asarray(index, dtype=np.uint64)
    out = np.empty((len(index), n))
    a0, a1 = normal_pairs(anc_words[:, 2], anc_words[:, 3])
    out[:, 0] = a0
    if n > 1:
        out[:, 1] = a1
    if n > 2:
        out[:, 2:] = normals(index, slot0, n - 2, generation, seed)
    return out


def prior_logpdf(theta, kinds, params):
    """Product prior in log space with scipy's closed-support pdfs."""
    theta = np.atleast_2d(theta)
    lp = np.zeros(len(theta))
    with np.errstate(divide="ignore"):
        for k, (kind, p) in enumerate(zip(kinds, params)):
            x = theta[:, k]
            if kind == "flat":
                continue
            if kind == "norm":
                lp += stats.norm.logpdf(x, p[0], p[1])
            elif kind == "uniform":
                lp += np.log(stats.uniform.pdf(x, p[0], p[1]))
            elif kind == "expon":
                lp += np.log(stats.expon.pdf(x, p[0], p[1]))
            elif kind == "laplace":
                lp += stats.laplace.logpdf(x, p[0], p[1])
            elif kind == "lognorm":
                # logpdf, not log(pdf): for a wide s the density next to loc
                # exceeds the largest double while its log is ~700.  scipy
                # takes log(s y sqrt(2 pi)) of a product that overflows for
                # y near the largest double and is rounded for a subnormal
                # one: there the same density through scipy's normal,
                # log f(y) = norm.logpdf(log y; 0, s) - log y
                with np.errstate(all="ignore"):
                    l = stats.lognorm.logpdf(x, p[0], p[1], p[2])
                    y = (x - p[1]) / p[2]
                    edge = (y > 0) & np.isfinite(y) & ((y < 1e-290) | (y > 1e290))
                    l[edge] = (stats.norm.logpdf(np.log(y[edge]), 0.0, p[0])
                               - np.log(y[edge]) - np.log(p[2]))
                lp += l
            elif kind == "gamma":
                lp += np.log(stats.gamma.pdf(x, p[0], p[1], p[2]))
            elif kind == "beta":
                lp += np.log(stats.beta.pdf(x, p[0], p[1], p[2], p[3]))
            else:
                raise ValueError(kind)
    return lp


def propose_local(X, w, chol, seed, generation, idx0, B, kinds=None, params=None,
                  max_attempts=1000):
    """Device abc_local_propose replayed (LocalTransition.rvs,
    pyabc/transition/local_transition.py:141-145: j ~ Cat(w), theta ~
    N(X_j, cov_j)): theta = X_j + chol_j n with the per-particle Cholesky
    factor chol [N, d, d]; same Philox streams and re-draw loop as
    propose_mvn."""
    return propose_mvn(X, w, chol, seed, generation, idx0, B, kinds, params,
                       max_attempts, per_particle=True)


def propose_mvn(X, w, L, seed, generation, idx0, B, kinds=None, params=None,
                max_attempts=1000, per_particle=False):
    """Device abc_propose replayed: returns theta, prior logpdf, ancestor,
    attempts."""
    X = np.asarray(X, dtype=np.float64)
    N, d = X.shape
    cdf = np.cumsum(np.asarray(w, dtype=np.float64))
    total = cdf[-1]
    kinds = kinds or ["flat"] * d
    params = params if params is not None else np.zeros((d, 4))
    idx = np.arange(idx0, idx0 + B, dtype=np.uint64)
    theta = np.empty((B, d))
    lp = np.full(B, -np.inf)
    anc = np.empty(B, dtype=np.int64)
    att = np.full(B, max_attempts + 1, dtype=np.int64)
    todo = np.ones(B, dtype=bool)
    for a in range(max_attempts):
        if not todo.any():
            break
        ii = idx[todo]
        s0 = a * SLOTS_PER_ATTEMPT
        r = philox4x32_10(ii, s0, generation, seed)
        u = uniform53(r[:, 0], r[:, 1])
        j = np.minimum(np.searchsorted(cdf, u * total, side="right"), N - 1)
        n = perturbation_normals(ii, s0 + SLOT_PERTURB, d, generation, seed, r)
        if per_particle:
            th = X[j] + np.einsum("bkq,bq->bk", np.asarray(L)[j], n)
        else:
            th = X[j] + n @ np.asarray(L).T
        l = prior_logpdf(th, kinds, params)
        pos = np.nonzero(todo)[0]
        theta[pos], lp[pos], anc[pos] = th, l, j
        ok = l > -np.inf
        att[pos[ok]] = a + 1
        todo[pos[ok]] = False
    return theta, lp, anc, att


def gamma_draws(a, index, base, generation, seed):
    """Device gamma_draw replayed (pyabc_amd/csrc/abc_candidate.h): one
    Marsaglia-Tsang gamma(a, 1) draw per candidate, iteration `it` from slot
    base + it (normal = first Box-Muller value of words 0, 1; accept uniform
    = word 2); for a < 1 the boost u^(1/a) from word 0 of slot base + 500 and
    the draw of a + 1.  Returns (draw, margin): margin is the smallest
    |log u - rhs| over the accept tests the candidate met -- the only
    decisions that depend on the device's log."""
    index = np.asarray(index, dtype=np.uint64)
    n = len(index)
    a = float(a)
    boost = np.ones(n)
    if a < 1.0:
        r = philox4x32_10(index, base + 500, generation, seed)
        boost = uniform01(r[:, 0]) ** (1.0 / a)
        a += 1.0
    dd = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * dd)
    out = dd * boost            # the device's value after 480 rejections
    margin = np.full(n, np.inf)
    todo = np.ones(n, dtype=bool)
    for it in range(480):
        pos = np.nonzero(todo)[0]
        if len(pos) == 0:
            break
        r = philox4x32_10(index[pos], base + it, generation, seed)
        n0, _ = normal_pairs(r[:, 0], r[:, 1])
        v = 1.0 + c * n0
        live = v > 0.0
        v = np.where(live, v, 1.0)
        v = v * v * v
        lu = np.log(uniform01(r[:, 2]))
        rhs = 0.5 * n0 * n0 + dd - dd * v + dd * np.log(v)
        margin[pos[live]] = np.minimum(margin[pos[live]], np.abs(lu - rhs)[live])
        acc = live & (lu < rhs)
        out[pos[acc]] = dd * v[acc] * boost[pos[acc]]
        todo[pos[acc]] = False
    return out, margin


def prior_draws(kind, p, index, base, generation, seed):
    """Device prior_draw1 replayed for one coordinate: (draw, margin) of the
    candidates `index` from the streams at slot `base` (gamma: base + 1 + it;
    beta: a second gamma stream at base + 1 + 256 + it).  margin as in
    gamma_draws (inf for the kinds that make no accept decision)."""
    index = np.asarray(index, dtype=np.uint64)
    inf = np.full(len(index), np.inf)
    if kind == "gamma":
        x, m = gamma_draws(p[0], index, base + 1, generation, seed)
        return p[1] + p[2] * x, m
    if kind == "beta":
        x, mx = gamma_draws(p[0], index, base + 1, generation, seed)
        y, my = gamma_draws(p[1], index, base + 1 + 256, generation, seed)
        return p[2] + p[3] * x / (x + y), np.minimum(mx, my)
    r = philox4x32_10(index, base, generation, seed)
    if kind == "norm":
        n0, _ = normal_pairs(r[:, 0], r[:, 1])
        return p[0] + p[1] * n0, inf
    if kind == "uniform":
        return p[0] + p[1] * uniform53(r[:, 0], r[:, 1]), inf
    if kind == "expon":
        return p[0] - p[1] * np.log(uniform01(r[:, 0])), inf
    if kind == "laplace":
        u = uniform01(r[:, 0]) - 0.5
        return p[0] - p[1] * np.copysign(1.0, u) * np.log1p(-2.0 * np.abs(u)), inf
    if kind == "lognorm":
        n0, _ = normal_pairs(r[:, 0], r[:, 1])
        with np.errstate(over="ignore", under="ignore"):
            return p[1] + p[2] * np.exp(p[0] * n0), inf
    raise ValueError(kind)


def propose_prior(kinds, params, seed, generation, idx0, B, max_attempts=1000):
    """Device abc_propose with X == nullptr replayed (PROP_PRIOR, the t = 0
    proposal, smc.py:624-626: theta = prior.rvs()): coordinate k of attempt a
    from slot a * 65536 + SLOT_PRIOR + 512 k, the whole row re-drawn while
    the prior density (scipy's, prior_logpdf) is 0.  Returns theta, prior
    logpdf, attempts (max_attempts + 1: every attempt left the support; theta
    is then the last one, logpdf -inf) and the smallest accept margin of the
    row's gamma / beta draws over all its attempts."""
    params = np.asarray(params, dtype=np.float64)
    d = len(kinds)
    idx = np.arange(idx0, idx0 + B, dtype=np.uint64)
    theta = np.empty((B, d))
    lp = np.full(B, -np.inf)
    att = np.full(B, max_attempts + 1, dtype=np.int64)
    margin = np.full(B, np.inf)
    todo = np.ones(B, dtype=bool)
    for a in range(max_attempts):
        pos = np.nonzero(todo)[0]
        if len(pos) == 0:
            break
        th = np.empty((len(pos), d))
        for k in range(d):
            base = a * SLOTS_PER_ATTEMPT + SLOT_PRIOR + 512 * k
            th[:, k], m = prior_draws(kinds[k], params[k], idx[pos], base, generation, seed)
            margin[pos] = np.minimum(margin[pos], m)
        l = prior_logpdf(th, kinds, params)
        theta[pos] = th
        ok = l > -np.inf
        lp[pos[ok]] = l[ok]
        att[pos[ok]] = a + 1
        todo[pos[ok]] = False
    return theta, lp, att, margin


def prior_uniforms(index, att, k, generation, seed):
    """The (0, 1) uniform of candidate `index`'s prior stream for dimension
    k in the attempt it accepted (device abc_prior_uniforms): words 0..1 of
    slot (att - 1) * 65536 + SLOT_PRIOR + 512 k, 53 bits plus a half.  An
    ABC_PRIOR_HOST coordinate's t = 0 draw is scipy's ppf of it."""
    index = np.asarray(index, dtype=np.uint64)
    att = np.maximum(np.asarray(att, dtype=np.int64) - 1, 0)
    out = np.empty(index.shape)
    for a in np.unique(att):
        sel = att == a
        r = philox4x32_10(index[sel], int(a) * SLOTS_PER_ATTEMPT + SLOT_PRIOR + 512 * k,
                          generation, seed)
        hi = (r[:, 0] >> np.uint32(5)).astype(np.float64)
        lo = (r[:, 1] >> np.uint32(6)).astype(np.float64)
        out[sel] = (hi * 67108864.0 + lo + 0.5) / 9007199254740992.0
    return out


def simulate_linear_gaussian(theta, src, a, sigma, seed, generation, idx0):
    """x[b, k] = a[k] theta[b, src[k]] + sigma[k] n_k (normal k of the
    candidate's simulation stream)."""
    theta = np.atleast_2d(theta)
    B = len(theta)
    S = len(src)
    idx = np.arange(idx0, idx0 + B, dtype=np.uint64)
    n = normals(idx, SLOT_SIM, S, generation, seed)
    return np.asarray(a)[None, :] * theta[:, np.asarray(src)] + \
        np.asarray(sigma)[None, :] * n
