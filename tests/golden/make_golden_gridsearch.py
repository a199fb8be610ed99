"""Generate tests/golden/gridsearch.npz by importing the pyABC 0.10.5 reference.

Runs in the build container only, with the reference checkout and this
directory on PYTHONPATH (like make_golden_scales.py); never on the GPU box,
and nothing here is imported by the product.

    PYTHONDONTWRITEBYTECODE=1 OMP_NUM_THREADS=1 \
      PYTHONPATH=<pyabc 0.10.5 checkout>:tests/golden \
      python tests/golden/make_golden_gridsearch.py

Each case runs what pyabc/transition/model_selection.py:9-74 reduces to once
the ``iid`` keyword (gone from scikit-learn) is left out:

    sklearn.model_selection.GridSearchCV(
        pyabc.transition.MultivariateNormalTransition(), grid, cv=k,
        return_train_score=True, error_score='raise').fit(X, w)

with X a DataFrame of correlated Gaussian rows and w Gamma(1) weights,
normalised.  Per case {c}:

    {c}__X [N, d], {c}__w [N], {c}__cv, {c}__scaling [nc] and
    {c}__selector [nc] (the candidates in ParameterGrid order),
    {c}__test [nc, k], {c}__train [nc, k] (split scores),
    {c}__mean_test, __std_test, __rank_test, __mean_train, __std_train [nc],
    {c}__best_index, {c}__cov [d, d] (the refit),
    {c}__fold0_logpdf [nc, n_test_0] (log density of fold 0's held-out rows)

A  N = 103, d = 3, default grid, cv = 5 (folds 21, 21, 21, 20, 20)
Aiso  A with the weights of the last fold's train rows summing to 1 + 5e-7:
   TransitionMeta.wrap_fit's np.isclose branch that skips the normalisation
B  N = 64, d = 1, grid [0.3], cv = 4
C  N = 257, d = 10, 13 scalings geomspace(0.02, 4), cv = 3
D  A with a quarter of the weights 0
E  A with row E__row moved out until its held-out log density at scaling
   0.05 is about -300: finite in fp64, far below the f32 exp2 range
F  A with the same row moved farther: its fold's score is -inf
G  N = 40, d = 3, cv = 5, scaling x bandwidth_selector (at d = 2 the two
   rules are the same number, n^(-1/6), and the winner would be a tie)
H3 N = 3, d = 1, cv = 5 reduced to 3 (the wrapper's rule);  H1 N = 1: the
   estimator's own fit (H1__cov only)
"""
import os
import warnings

import numpy as np
import pandas as pd
from scipy.special import logsumexp

import stub_env  # noqa: F401  (must precede pyabc)
from sklearn.model_selection import GridSearchCV, KFold, ParameterGrid
from pyabc.transition import (MultivariateNormalTransition,
                              scott_rule_of_thumb, silverman_rule_of_thumb)

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_GRID = {"scaling": np.linspace(0.05, 1.0, 5)}
ISCLOSE_EDGE = 1e-8 + 1e-5
SELECTORS = {silverman_rule_of_thumb: "silverman", scott_rule_of_thumb: "scott"}
F64_DENORMAL = (-760.0, -700.0)   # log densities here lose bits to underflow


def population(seed, N, d):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(d, d)) + 2 * np.eye(d)
    X = rng.normal(size=(N, d)) @ A.T + rng.normal(size=d)
    w = rng.gamma(1.0, size=N)
    return X, w / w.sum()


def frame(X):
    return pd.DataFrame(X, columns=[f"p{k}" for k in range(X.shape[1])])


def held_out_logpdf(X, w, cv, params, fold):
    """Log density of the fold's test rows under the fit to its train rows,
    term by term in log space (no underflow)."""
    train, test = list(KFold(cv).split(X))[fold]
    est = MultivariateNormalTransition(**params)
    est.fit(frame(X[train]), w[train].copy())
    lw = np.log(est.w, out=np.full(len(train), -np.inf), where=est.w > 0)
    return np.array([logsumexp(est.normal.logpdf(x - X[train]) + lw)
                     for x in X[test]])


def run(res, c, X, w, grid, cv, check_winner):
    X, w = X.copy(), w.copy()
    res[f"{c}__X"], res[f"{c}__w"], res[f"{c}__cv"] = X.copy(), w.copy(), cv
    cands = list(ParameterGrid(grid))
    for train, _ in KFold(cv).split(X):
        s = w[train].sum()
        if c == "Aiso" and train[-1] < len(X) - 1:
            assert 0 < abs(s - 1) < 1e-6, s            # the dedicated fold
        else:
            assert abs(abs(s - 1) - ISCLOSE_EDGE) > 1e-4, (c, s)
    gs = GridSearchCV(MultivariateNormalTransition(), grid, cv=cv,
                      return_train_score=True, error_score="raise")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with np.errstate(divide="ignore", invalid="ignore"):
            gs.fit(frame(X), w)
    r = gs.cv_results_
    assert r["params"] == cands
    res[f"{c}__scaling"] = np.array([p.get("scaling", 1.0) for p in cands], dtype=np.float64)
    res[f"{c}__selector"] = np.array(
        [SELECTORS[p.get("bandwidth_selector", silverman_rule_of_thumb)] for p in cands])
    for kind in ("test", "train"):
        res[f"{c}__{kind}"] = np.stack(
            [r[f"split{f}_{kind}_score"] for f in range(cv)], axis=1)
        res[f"{c}__mean_{kind}"] = r[f"mean_{kind}_score"]
        res[f"{c}__std_{kind}"] = r[f"std_{kind}_score"]
    res[f"{c}__rank_test"] = r["rank_test_score"]
    res[f"{c}__best_index"] = gs.best_index_
    res[f"{c}__cov"] = np.atleast_2d(gs.best_estimator_.cov)
    lp0 = np.stack([held_out_logpdf(X, res[f"{c}__w"], cv, p, 0) for p in cands])
    res[f"{c}__fold0_logpdf"] = lp0
    # the recorded fold-0 scores are those densities' weighted sums
    n0 = lp0.shape[1]
    fin = np.isfinite(res[f"{c}__test"][:, 0])
    assert np.allclose((lp0 * res[f"{c}__w"][:n0]).sum(axis=1)[fin],
                       res[f"{c}__test"][fin, 0], rtol=1e-9, atol=1e-9), c
    # no held-out density in fp64's denormal band, where the reference's own
    # sum has lost precision
    for f in range(cv):
        for p in cands:
            lp = held_out_logpdf(X, res[f"{c}__w"], cv, p, f)
            assert not np.any((lp > F64_DENORMAL[0]) & (lp < F64_DENORMAL[1])), (c, f, p)
    if check_winner:
        m = np.sort(r["mean_test_score"])[::-1]
        assert m[0] - m[1] > 1e-4, (c, m[:2])
    return gs


def move_row(X, w, row, target_lo, target_hi):
    """X with `row` (in fold 0) moved along the first axis until its held-out
    log density at scaling 0.05 lies in [target_lo, target_hi]."""
    lo, hi = 0.0, 1e4
    for _ in range(200):
        t = 0.5 * (lo + hi)
        Y = X.copy()
        Y[row, 0] += t
        lp = held_out_logpdf(Y, w, 5, {"scaling": 0.05}, 0)[row]
        if lp > target_hi:
            lo = t
        elif lp < target_lo:
            hi = t
        else:
            return Y, lp
    raise AssertionError("no displacement found")


def gen():
    res = {}
    XA, wA = population(2024, 103, 3)
    run(res, "A", XA, wA, DEFAULT_GRID, 5, True)

    w = wA.copy()
    w[:83] *= (1 + 5e-7) / w[:83].sum()
    run(res, "Aiso", XA, w, DEFAULT_GRID, 5, False)

    XB, wB = population(7, 64, 1)
    run(res, "B", XB, wB, {"scaling": [0.3]}, 4, False)

    XC, wC = population(99, 257, 10)
    run(res, "C", XC, wC, {"scaling": np.geomspace(0.02, 4, 13)}, 3, True)

    w = wA.copy()
    w[np.random.default_rng(5).permutation(103)[:26]] = 0.0
    run(res, "D", XA, w / w.sum(), DEFAULT_GRID, 5, True)

    row = 5
    XE, lpE = move_row(XA, wA, row, -320.0, -280.0)
    assert -600 <= lpE <= -100
    # below the f32 exp2 range (2^-126) relative to the largest weight
    assert lpE - np.log(wA.max()) < -126 * np.log(2) - 50
    run(res, "E", XE, wA, DEFAULT_GRID, 5, False)
    res["E__row"] = row
    assert np.isclose(res["E__fold0_logpdf"][0, row], lpE)
    assert np.all(np.isfinite(res["E__test"][:, 0]))

    XF, lpF = move_row(XA, wA, row, -8800.0, -8400.0)
    run(res, "F", XF, wA, DEFAULT_GRID, 5, False)
    res["F__row"] = row
    assert res["F__test"][0, 0] == -np.inf

    XG, wG = population(31, 40, 3)
    run(res, "G", XG, wG,
        {"scaling": [0.3, 0.6, 1.0],
         "bandwidth_selector": [silverman_rule_of_thumb, scott_rule_of_thumb]},
        5, True)

    XH, wH = population(13, 3, 1)
    run(res, "H3", XH, wH, DEFAULT_GRID, 3, False)
    res["H3__cv"] = 5                      # what the caller asks for
    X1 = np.array([[0.7, -1.3]])
    est = MultivariateNormalTransition()
    est.fit(frame(X1), np.array([1.0]))
    res["H1__X"], res["H1__w"], res["H1__cov"] = X1, np.array([1.0]), est.cov

    path = os.path.join(HERE, "gridsearch.npz")
    np.savez_compressed(path, **res)
    print("gridsearch", len(res), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    gen()
