"""Generate tests/golden/kde.npz by importing the pyABC 0.10.5 reference.

Runs in the build container only, with the reference checkout and this
directory on PYTHONPATH (like make_golden_gridsearch.py); never on the GPU
box, and nothing here is imported by the product.

    PYTHONDONTWRITEBYTECODE=1 OMP_NUM_THREADS=1 MPLBACKEND=Agg \
      PYTHONPATH=<pyabc 0.10.5 checkout>:tests/golden \
      python tests/golden/make_golden_kde.py

Each case {c} is a population and the panels pyabc.visualization.kde_1d /
kde_2d (kde.py:19-74, 174-248) compute for it, with kde =
MultivariateNormalTransition(scaling, bandwidth_selector):

    {c}__X [N, d], {c}__w [N] (normalised), {c}__limits [d, 2] (NaN = None),
    {c}__numx, {c}__numy, {c}__scaling, {c}__rule ("silverman" / "scott"),
    {c}__panels: the panel keys, "p0" or "p0|p1" (x|y), and per key {k}
    {c}__x__{k} (kde_1d's x, or kde_2d's X[0]), {c}__y__{k} (Y[:, 0]),
    {c}__pdf__{k} ([numx] or [numy, numx]), {c}__cov__{k} (the fitted kde.cov)

A  d = 1, N = 257
B  d = 3, N = 1000, Gamma(1) weights, limits given for p1 only: the whole
   KDE matrix (p0, p0|p1, p1, p0|p2, p1|p2, p2); also the credible bounds
   B__ci [d, 2 levels, 2] at levels 0.5 and 0.95 (compute_credible_interval)
   and the medians B__median [d]
C  a pair with correlation 0.999, N = 300
D  columns at scales 1e-3 and 1e4, both with a mean offset of 1e6, N = 300
E  d = 2, N = 400, a quarter of the weights 0
F7 E's population on a 7 x 13 grid;  F1 its 1-D panels on a one-point grid
G  E's population with limits 40 standard deviations out: part of the
   reference densities are exactly 0
H  d = 3, N = 120: p1 constant, p2 a copy of p0 (the singular route):
   panels p1, p0|p1, p0|p2
I  N = 1, d = 2
J  d = 2, N = 150, scaling = 0.3 with the Scott rule
K  d = 2, N = 200: compute_kde_max (credible.py:376-384): K__kde_max_index
   and K__kde_vals [N], the densities at the particles
"""
import os

import numpy as np
import pandas as pd

import stub_env  # noqa: F401  (must precede pyabc)
from pyabc.transition import (MultivariateNormalTransition,
                              scott_rule_of_thumb, silverman_rule_of_thumb)
from pyabc.visualization.kde import kde_1d, kde_2d
from pyabc.visualization.credible import (compute_credible_interval,
                                          compute_kde_max, compute_quantile)

HERE = os.path.dirname(os.path.abspath(__file__))
RULES = {"silverman": silverman_rule_of_thumb, "scott": scott_rule_of_thumb}


def population(seed, N, d, gamma=True):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(d, d)) + 2 * np.eye(d)
    X = rng.normal(size=(N, d)) @ A.T + rng.normal(size=d)
    w = rng.gamma(1.0, size=N) if gamma else np.ones(N)
    return X, w / w.sum()


def frame(X):
    return pd.DataFrame(X, columns=[f"p{k}" for k in range(X.shape[1])])


def matrix_keys(d):
    keys = []
    for i in range(d):
        keys.append(f"p{i}")
        keys.extend(f"p{j}|p{i}" for j in range(i))
    return keys


def run(res, c, X, w, keys=None, limits=None, numx=50, numy=50, scaling=1.0,
        rule="silverman"):
    d = X.shape[1]
    df = frame(X)
    lim = np.full((d, 2), np.nan)
    for k, v in (limits or {}).items():
        lim[int(k[1:])] = [np.nan if b is None else b for b in v]
    keys = matrix_keys(d) if keys is None else keys
    res[f"{c}__X"], res[f"{c}__w"], res[f"{c}__limits"] = X.copy(), w.copy(), lim
    res[f"{c}__numx"], res[f"{c}__numy"] = numx, numy
    res[f"{c}__scaling"], res[f"{c}__rule"] = float(scaling), rule
    res[f"{c}__panels"] = np.array(keys)

    def lims(name):
        a, b = lim[int(name[1:])]
        return (None if np.isnan(a) else a), (None if np.isnan(b) else b)

    for key in keys:
        kde = MultivariateNormalTransition(scaling=scaling,
                                           bandwidth_selector=RULES[rule])
        names = key.split("|")
        with np.errstate(all="ignore"):
            if len(names) == 1:
                lo, hi = lims(names[0])
                x, pdf = kde_1d(df, w.copy(), names[0], xmin=lo, xmax=hi, numx=numx,
                                kde=kde)
                res[f"{c}__x__{key}"] = x
                res[f"{c}__pdf__{key}"] = np.atleast_1d(np.asarray(pdf, dtype=np.float64))
            else:
                (xl, xh), (yl, yh) = lims(names[0]), lims(names[1])
                Xg, Yg, PDF = kde_2d(df, w.copy(), names[0], names[1], xmin=xl,
                                     xmax=xh, ymin=yl, ymax=yh, numx=numx,
                                     numy=numy, kde=kde)
                res[f"{c}__x__{key}"], res[f"{c}__y__{key}"] = Xg[0], Yg[:, 0]
                res[f"{c}__pdf__{key}"] = np.asarray(PDF, dtype=np.float64).reshape(Xg.shape)
        res[f"{c}__cov__{key}"] = np.atleast_2d(kde.cov)


def gen():
    res = {}
    XA, wA = population(11, 257, 1)
    run(res, "A", XA, wA)

    XB, wB = population(2024, 1000, 3)
    lo, hi = XB[:, 1].min(), XB[:, 1].max()
    run(res, "B", XB, wB, limits={"p1": (lo - 1.0, hi + 2.0)})
    ci = np.empty((3, 2, 2))
    for k in range(3):
        for j, level in enumerate((0.5, 0.95)):
            ci[k, j] = compute_credible_interval(XB[:, k], wB, level)
    res["B__ci"] = ci
    res["B__median"] = np.array([compute_quantile(XB[:, k], wB, 0.5) for k in range(3)])

    rng = np.random.default_rng(3)
    z = rng.normal(size=(300, 2))
    rho = 0.999
    XC = np.stack([z[:, 0], rho * z[:, 0] + np.sqrt(1 - rho ** 2) * z[:, 1]], axis=1)
    wC = rng.gamma(1.0, size=300)
    run(res, "C", XC, wC / wC.sum(), keys=["p0|p1"])
    assert np.corrcoef(XC.T)[0, 1] > 0.998

    z = rng.normal(size=(300, 2))
    XD = np.stack([1e6 + 1e-3 * z[:, 0], 1e6 + 1e4 * (0.5 * z[:, 0] + z[:, 1])], axis=1)
    wD = rng.gamma(1.0, size=300)
    run(res, "D", XD, wD / wD.sum())

    XE, wE = population(5, 400, 2)
    wE[np.random.default_rng(6).permutation(400)[:100]] = 0.0
    wE /= wE.sum()
    run(res, "E", XE, wE)
    run(res, "F7", XE, wE, numx=7, numy=13)
    # (kde_2d itself cannot take a 1 x 1 grid: its pdf is then a float, which
    # has no reshape; the 1-D panels carry the one-point grid)
    run(res, "F1", XE, wE, keys=["p0", "p1"], numx=1, numy=1)

    sd = XE.std(axis=0)
    mu = XE.mean(axis=0)
    run(res, "G", XE, wE, numx=40, numy=40,
        limits={f"p{k}": (mu[k] - 40 * sd[k], mu[k] + 40 * sd[k]) for k in range(2)})
    assert np.any(res["G__pdf__p0|p1"] == 0.0) and np.any(res["G__pdf__p0|p1"] > 1e-3)
    assert np.any(res["G__pdf__p0"] == 0.0)

    XH, wH = population(8, 120, 1)
    XH = np.concatenate([XH, np.full((120, 1), 2.5), XH], axis=1)
    run(res, "H", XH, wH, keys=["p1", "p0|p1", "p0|p2"], numx=9, numy=11,
        limits={"p1": (2.0, 3.0)})

    run(res, "I", np.array([[0.7, -1.3]]), np.array([1.0]), numx=9, numy=11,
        limits={"p0": (0.0, 1.5), "p1": (-2.5, 0.0)})

    XJ, wJ = population(21, 150, 2)
    run(res, "J", XJ, wJ, scaling=0.3, rule="scott", numx=20, numy=30)

    XK, wK = population(33, 200, 2)
    kde = MultivariateNormalTransition()
    pnt = compute_kde_max(kde, frame(XK), wK.copy())
    vals = np.array([kde.pdf(p) for _, p in frame(XK).iterrows()])
    ix = int(np.flatnonzero((XK == pnt.values[None, :]).all(axis=1))[0])
    assert ix == int(np.argmax(vals))
    top = np.sort(vals)[::-1]
    assert (top[0] - top[1]) / top[0] > 1e-5, top[:2]
    res["K__X"], res["K__w"] = XK, wK
    res["K__kde_max_index"], res["K__kde_vals"] = ix, vals

    path = os.path.join(HERE, "kde.npz")
    np.savez_compressed(path, **res)
    print("kde", len(res), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    gen()
