"""float64 numpy restatement of the scaled KDE and of the grid search built on
it (tests only; imports neither the product nor pyABC).

pyabc/transition/multivariatenormal.py:72-113 and model_selection.py:9-74:
cov = np.cov(X, aweights=w) * bw(ESS, d)^2 * scaling, pdf(x) = sum_j w_j
N(x - X_j; 0, cov), score = sum_i w_i log pdf(x_i), KFold(k) without shuffle.
The densities are evaluated term by term in log space over explicit
differences; a value below ln 2^-1075, where every term of the reference's
linear-space fp64 sum has rounded to zero, is reported as -inf as np.log(0.)
does.
"""
import numpy as np
from scipy.special import logsumexp

LOG_2PI = float(np.log(2 * np.pi))
LOG_F64_UNDERFLOW = -1075 * float(np.log(2))


def bandwidth(rule, ess, d):
    """multivariatenormal.py:14-37."""
    if rule == "scott":
        return ess ** (-1.0 / (d + 4))
    return (4 / ess / (d + 2)) ** (1 / (d + 4))


def whitening(cov):
    """U with U U^T = cov^-1 and log det cov (full rank)."""
    s, u = np.linalg.eigh(np.atleast_2d(cov))
    return u / np.sqrt(s), float(np.sum(np.log(s)))


def fit(X, w, rule="silverman"):
    """(mean, cov at scaling 1) of a weighted population; w as the estimator
    holds it (normalised or not: np.cov and the mean do not care, ESS does)."""
    d = X.shape[1]
    mu = np.average(X, axis=0, weights=w)
    cov = np.atleast_2d(np.cov(X, aweights=w, rowvar=False))
    return mu, cov * bandwidth(rule, 1 / np.sum(w ** 2), d) ** 2


def log_consts(d, log_det, scalings):
    return -0.5 * (d * LOG_2PI + log_det + d * np.log(np.asarray(scalings, dtype=np.float64)))


def scaled_logpdf(x, X, w, U, scalings, lc, block=64):
    """out [G, M]: log sum_j w_j exp(-|(x_i - X_j) U|^2 / (2 s_g)) + lc[g]."""
    scalings = np.asarray(scalings, dtype=np.float64)
    with np.errstate(divide="ignore"):
        lw = np.log(w)
    out = np.empty((len(scalings), len(x)))
    for i0 in range(0, len(x), block):
        diff = x[i0:i0 + block, None, :] - X[None, :, :]
        maha = np.sum((diff @ U) ** 2, axis=2)             # [m, N]
        for g, s in enumerate(scalings):
            out[g, i0:i0 + block] = logsumexp(-0.5 * maha / s + lw[None, :], axis=1) + lc[g]
    out[out < LOG_F64_UNDERFLOW] = -np.inf
    return out


def score(out, wt):
    with np.errstate(invalid="ignore"):
        return (out * wt[None, :]).sum(axis=1)


def kfold(n, k):
    """(train, test) index arrays of KFold(k) without shuffle, written out."""
    idx = np.arange(n)
    start = 0
    for f in range(k):
        size = n // k + (1 if f < n % k else 0)
        test = idx[start:start + size]
        yield np.concatenate((idx[:start], idx[start + size:])), test
        start += size


def grid_search(X, w, scalings, cv, rule="silverman", train_score=False):
    """test [G, k] (and train) scores of the search, TransitionMeta.wrap_fit's
    conditional normalisation of the train weights included."""
    d = X.shape[1]
    test = np.empty((len(scalings), cv))
    train = np.empty_like(test) if train_score else None
    for f, (tr, te) in enumerate(kfold(len(X), cv)):
        wtr = w[tr].copy()
        if not np.isclose(wtr.sum(), 1):
            wtr /= wtr.sum()
        mu, cov = fit(X[tr], wtr, rule)
        U, log_det = whitening(cov)
        lc = log_consts(d, log_det, scalings)
        test[:, f] = score(scaled_logpdf(X[te], X[tr], wtr, U, scalings, lc), w[te])
        if train_score:
            train[:, f] = score(scaled_logpdf(X[tr], X[tr], wtr, U, scalings, lc), wtr)
    return test, train
