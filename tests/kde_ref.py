"""float64 numpy restatement of the marginal KDEs on plot grids and of the
credible-interval functions (tests only; imports neither the product nor
pyABC).

pyabc/visualization/kde.py:19-74, 174-248: fit a MultivariateNormalTransition
to one or two columns -- cov = np.cov(X, aweights=w) * bw(ESS, k)^2 * scaling
(smart_cov: diag(|x|) when N = 1), frozen scipy mvn(cov, allow_singular=True)
-- and evaluate pdf(g) = sum_j w_j N(g - X_j; 0, cov) on linspace / meshgrid
grids.  pyabc/visualization/credible.py:356-392 for the quantiles and the MAP
index.  The densities are computed term by term in log space over explicit
differences with an exact log-sum-exp, so they stay meaningful where the
reference's plain fp64 sum has underflowed to 0.
"""
import numpy as np
from scipy.special import logsumexp

LOG_2PI = float(np.log(2 * np.pi))


def bandwidth(rule, ess, k):
    """multivariatenormal.py:14-37."""
    if rule == "scott":
        return ess ** (-1.0 / (k + 4))
    return (4 / ess / (k + 2)) ** (1 / (k + 4))


def fit_cov(Xc, w, scaling=1.0, rule="silverman"):
    """The KDE covariance of the columns Xc [N, k] (multivariatenormal.py:72-82)."""
    N, k = Xc.shape
    if N == 1:
        sample = np.diag(np.abs(Xc[0]))
    else:
        sample = np.atleast_2d(np.cov(Xc, aweights=w, rowvar=False))
    return sample * bandwidth(rule, 1 / np.sum(w ** 2), k) ** 2 * scaling


def psd(cov):
    """scipy.stats._multivariate._PSD: (U, V, log_pdet, support tolerance)."""
    s, u = np.linalg.eigh(np.atleast_2d(cov))
    eps = 1e6 * np.finfo(np.float64).eps * np.max(np.abs(s))
    keep = s > eps
    return u[:, keep] / np.sqrt(s[keep]), u[:, ~keep], float(np.sum(np.log(s[keep]))), 1e3 * eps


def log_kde(pts, Xc, w, cov, block=None):
    """log sum_j w_j N(pts_i - Xc_j; 0, cov) [M]; -inf where every term is 0
    (zero weights; outside the support of a singular cov)."""
    block = max(1, (1 << 21) // len(Xc)) if block is None else block
    U, V, log_pdet, tol = psd(cov)
    rank = U.shape[1]
    with np.errstate(divide="ignore"):
        lw = np.log(w)
    out = np.empty(len(pts))
    for i0 in range(0, len(pts), block):
        diff = pts[i0:i0 + block, None, :] - Xc[None, :, :]
        lt = -0.5 * np.sum((diff @ U) ** 2, axis=2) + lw[None, :]
        if V.shape[1]:
            lt = np.where(np.linalg.norm(diff @ V, axis=2) < tol, lt, -np.inf)
        out[i0:i0 + block] = logsumexp(lt, axis=1)
    return out - 0.5 * (rank * LOG_2PI + log_pdet)


def axes(X, names, key, limits, numx, numy):
    """The linspace axes of panel key (a tuple of one or two names)."""
    out = []
    for name, n in zip(key, (numx, numy)):
        c = names.index(name)
        a, b = (limits or {}).get(name, (None, None))
        out.append(np.linspace(X[:, c].min() if a is None else a,
                               X[:, c].max() if b is None else b, num=n))
    return out


def log_kde_1d(X, w, names, x, limits=None, numx=50, scaling=1.0, rule="silverman"):
    """(x_vals, log pdf [numx]) of kde_1d."""
    (xv,) = axes(X, names, (x,), limits, numx, 1)
    Xc = X[:, [names.index(x)]]
    return xv, log_kde(xv[:, None], Xc, w, fit_cov(Xc, w, scaling, rule))


def log_kde_2d(X, w, names, x, y, limits=None, numx=50, numy=50, scaling=1.0,
               rule="silverman"):
    """(X, Y, log PDF [numy, numx]) of kde_2d."""
    xv, yv = axes(X, names, (x, y), limits, numx, numy)
    Xg, Yg = np.meshgrid(xv, yv)
    Xc = X[:, [names.index(x), names.index(y)]]
    lp = log_kde(np.stack([Xg.ravel(), Yg.ravel()], axis=1), Xc, w,
                 fit_cov(Xc, w, scaling, rule))
    return Xg, Yg, lp.reshape(Xg.shape)


def matrix_keys(names):
    keys = []
    for i, n in enumerate(names):
        keys.append((n,))
        keys.extend((names[j], n) for j in range(i))
    return keys


def log_kde_matrix(X, w, names, limits=None, numx=50, numy=50, scaling=1.0,
                   rule="silverman"):
    """{key: log pdf array} for every panel of the KDE matrix."""
    res = {}
    for key in matrix_keys(names):
        if len(key) == 1:
            res[key] = log_kde_1d(X, w, names, key[0], limits, numx, scaling, rule)[1]
        else:
            res[key] = log_kde_2d(X, w, names, key[0], key[1], limits, numx, numy,
                                  scaling, rule)[2]
    return res


GOLDEN_CASES = ("A", "B", "C", "D", "E", "F7", "F1", "G", "H", "I", "J")


def golden_case(g, c):
    """Case c of tests/golden/kde.npz (make_golden_kde.py) as a dict: X, w,
    names, limits {name: (lo, hi)} with None for a missing bound, numx, numy,
    scaling, rule, keys (name tuples) and per key pdf, cov, x, y."""
    X = g[f"{c}__X"]
    names = [f"p{k}" for k in range(X.shape[1])]
    limits = {}
    for k, (a, b) in enumerate(g[f"{c}__limits"]):
        if not (np.isnan(a) and np.isnan(b)):
            limits[names[k]] = (None if np.isnan(a) else float(a),
                                None if np.isnan(b) else float(b))
    out = dict(X=X, w=g[f"{c}__w"], names=names, limits=limits,
               numx=int(g[f"{c}__numx"]), numy=int(g[f"{c}__numy"]),
               scaling=float(g[f"{c}__scaling"]), rule=str(g[f"{c}__rule"]),
               keys=[], pdf={}, cov={}, x={}, y={})
    for s in g[f"{c}__panels"]:
        key = tuple(str(s).split("|"))
        out["keys"].append(key)
        out["pdf"][key] = g[f"{c}__pdf__{s}"]
        out["cov"][key] = g[f"{c}__cov__{s}"]
        out["x"][key] = g[f"{c}__x__{s}"]
        if len(key) == 2:
            out["y"][key] = g[f"{c}__y__{s}"]
    return out


def log_panel(case, key):
    """The restated log density of one panel of a golden_case dict."""
    a = (case["X"], case["w"], case["names"])
    if len(key) == 1:
        return log_kde_1d(*a, key[0], case["limits"], case["numx"], case["scaling"],
                          case["rule"])[1]
    return log_kde_2d(*a, key[0], key[1], case["limits"], case["numx"], case["numy"],
                      case["scaling"], case["rule"])[2]


def quantile(vals, w, alpha):
    """weighted_statistics.py:20-29."""
    o = np.argsort(vals)
    v, ww = vals[o], w[o]
    return float(np.interp(alpha, np.cumsum(ww) - 0.5 * ww, v))


def credible_interval(vals, w, confidence):
    """credible.py:356-373."""
    if confidence <= 0.0 or confidence >= 1.0:
        raise ValueError(confidence)
    lb = 0.5 * (1.0 - confidence)
    return quantile(vals, w, lb), quantile(vals, w, confidence + lb)


def kde_max_index(X, w, scaling=1.0, rule="silverman"):
    """credible.py:376-384: (lowest index of the largest density, log
    densities at the particles)."""
    lp = log_kde(X, X, w, fit_cov(X, w, scaling, rule))
    return int(np.argmax(lp)), lp
