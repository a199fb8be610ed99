"""GridSearchCV on the device: abc_mvn_logpdf_scaled against the float64
restatement (tests/gridsearch_ref.py), the search against the pyABC 0.10.5
fixture (tests/golden/gridsearch.npz, made by make_golden_gridsearch.py),
the device route against sklearn's loop, and an ABCSMC run.

Tolerances: 2e-6 per log density, the figure include/abcgpu.h documents for
the f64-MFMA + f32-exp2 arithmetic; a score sum_i wt_i out_i then carries
2e-6 sum |wt|.  Measured maxima are in DESIGN.md (GridSearchCV section).
"""
import logging
import os

import numpy as np
import pandas as pd
import pytest

import gridsearch_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 2e-6
CAP = 8                       # grid points per launch (abc_mvn_scaled.hip GCAP)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "gridsearch.npz"))


def _dev(a):
    from pyabc_amd import gpu
    return gpu.as_dev(np.ascontiguousarray(a, dtype=np.float64))


def _population(seed, N, d, zero=False):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(d, d)) + 2 * np.eye(d)
    X = rng.normal(size=(N, d)) @ A.T + rng.normal(size=d)
    w = rng.gamma(1.0, size=N)
    if zero:
        w[rng.permutation(N)[:max(N // 4, 1)]] = 0.0
    return X, w / w.sum()


def _kernel_case(seed, M, N, d, G, zero=False):
    """Inputs of one kernel call and the restatement's answer: the KDE of a
    population of N rows (its covariance from a larger sample when N is too
    small to have one) at G scalings, at M points around it."""
    X, w = _population(seed, max(N, d + 5), d, zero)
    mu, cov = ref.fit(X, w)
    X, w = X[:N], w[:N]
    if zero and N > 1:
        w[0] = 0.0                                 # survives the cut
    if w.sum() == 0:
        w[:] = 1.0
    rng = np.random.default_rng(seed + 1)
    x = X[rng.integers(0, N, size=M)] + rng.normal(size=(M, d)) @ np.linalg.cholesky(cov).T
    wt = rng.gamma(1.0, size=M)
    s = np.geomspace(0.05, 2.0, G) if G > 1 else np.array([0.3])
    U, log_det = ref.whitening(cov)
    lc = ref.log_consts(d, log_det, s)
    out = ref.scaled_logpdf(x, X, w, U, s, lc)
    return dict(x=x, X=X, w=w, mu=mu, U=U, s=s, lc=lc, wt=wt, out=out,
                score=ref.score(out, wt))


def _run(c, sel=None, wt=True, X=None, w=None):
    from pyabc_amd import gpu
    sel = slice(None) if sel is None else sel
    out, score = gpu.mvn_logpdf_scaled(
        _dev(c["x"]), _dev(c["X"] if X is None else X), _dev(c["w"] if w is None else w),
        _dev(c["mu"]), _dev(c["U"]), c["s"][sel], c["lc"][sel],
        wt=_dev(c["wt"]) if wt else None)
    return out.cpu().numpy(), None if score is None else score.cpu().numpy()


# (M, N, d, G): the edges of M in {1, 15, 17, 300} x N in {1, 16, 103, 4099}
# x d in {1, 3, 4, 10, 25} x G in {1, 5, cap, cap + 1}: one point / one row,
# tiles short of and past 16, several blocks and chunks (N = 4099: 257 tiles),
# K blocks with and without padding (d = 3: 4 columns; d = 4: 5 -> 8), every
# G path (alone, 5, a full launch, a second launch of one)
SHAPES = [(1, 1, 1, 1), (15, 16, 3, 5), (17, 103, 4, CAP), (300, 4099, 10, CAP + 1),
          (17, 4099, 25, 5), (300, 103, 1, CAP + 1), (15, 1, 25, CAP), (1, 16, 10, 1),
          (300, 16, 3, 7), (17, 103, 3, 13)]


@pytest.mark.parametrize("M, N, d, G", SHAPES)
def test_kernel_against_restatement(M, N, d, G):
    c = _kernel_case(100 + M + N + d + G, M, N, d, G)
    out, score = _run(c)
    err = np.abs(out - c["out"]).max()
    serr = np.abs(score - c["score"]).max()
    print(f"scaled kernel M={M} N={N} d={d} G={G}: max |out - ref| = {err:.3e}, "
          f"max |score - ref| / sum|wt| = {serr / np.abs(c['wt']).sum():.3e}")
    assert np.all(np.isfinite(out))
    assert err <= TOL
    assert serr <= TOL * np.abs(c["wt"]).sum()
    # two runs: the same bits, scores included
    out2, score2 = _run(c)
    assert np.array_equal(out, out2) and np.array_equal(score, score2)
    # batching the grid changes no result: every g alone gives the same bits
    if G > 1:
        for g in range(G):
            og, sg = _run(c, slice(g, g + 1))
            assert np.array_equal(og[0], out[g]), g
            assert sg[0] == score[g], g
    # without wt there is no score and the densities are the same
    out3, none = _run(c, wt=False)
    assert none is None and np.array_equal(out3, out)


@pytest.mark.parametrize("M, N, d, G", [(17, 103, 3, 5), (300, 4099, 10, CAP + 1)])
def test_zero_weight_rows_contribute_nothing(M, N, d, G):
    c = _kernel_case(7, M, N, d, G, zero=True)
    assert (c["w"] == 0).sum() >= N // 5
    out, _ = _run(c)
    assert np.abs(out - c["out"]).max() <= TOL
    # the same population without those rows, and with them moved far away
    keep = c["w"] > 0
    out_cut, _ = _run(c, X=c["X"][keep], w=c["w"][keep])
    assert np.abs(out - out_cut).max() <= 2 * TOL
    Xfar = c["X"].copy()
    Xfar[~keep] += 1e3
    out_far, _ = _run(c, X=Xfar)
    assert np.array_equal(out_far, out)


def _fold0(z, c):
    """Fold 0 of a fixture case as the kernel sees it: held-out rows, train
    rows with the estimator's weights, the restatement's fit."""
    X, w, cv = z[f"{c}__X"], z[f"{c}__w"], int(z[f"{c}__cv"])
    tr, te = next(ref.kfold(len(X), cv))
    wtr = w[tr] / w[tr].sum()
    mu, cov = ref.fit(X[tr], wtr)
    U, log_det = ref.whitening(cov)
    s = z[f"{c}__scaling"]
    return dict(x=X[te], X=X[tr], w=wtr, mu=mu, U=U, s=s,
                lc=ref.log_consts(X.shape[1], log_det, s), wt=w[te])


def test_far_point_is_finite_and_within_tolerance(golden):
    """Case E: a held-out row ~25 kernel widths from every train row at
    scaling 0.05: log density about -318, below the f32 exp2 range relative
    to any fixed shift, finite in fp64."""
    c = _fold0(golden, "E")
    row = int(golden["E__row"])
    want = golden["E__fold0_logpdf"]
    assert -600 < want[0, row] < -100
    out, score = _run(c)
    print("case E far row:", out[:, row], "reference", want[:, row])
    assert np.all(np.isfinite(out))
    assert np.abs(out - want).max() <= TOL
    assert np.abs(out - ref.scaled_logpdf(c["x"], c["X"], c["w"], c["U"], c["s"],
                                          c["lc"])).max() <= TOL
    assert np.abs(score - golden["E__test"][:, 0]).max() <= TOL * c["wt"].sum()


def test_all_underflow_point_is_minus_inf_not_nan(golden):
    """Case F: every term of the reference's fp64 sum underflows at the three
    smallest scalings: -inf there (and in the score), finite at the others."""
    c = _fold0(golden, "F")
    row = int(golden["F__row"])
    want = golden["F__fold0_logpdf"]
    out, score = _run(c)
    assert not np.any(np.isnan(out)) and not np.any(np.isnan(score))
    assert np.all(out[:3, row] == -np.inf) and np.all(np.isfinite(out[3:, row]))
    others = np.arange(out.shape[1]) != row
    assert np.abs(out[:, others] - want[:, others]).max() <= TOL
    assert np.abs(out[3:, row] - want[3:, row]).max() <= TOL
    assert np.array_equal(score == -np.inf, golden["F__test"][:, 0] == -np.inf)
    # a weight of exactly 0 on that row: 0 * -inf is NaN, as numpy has it
    c["wt"] = c["wt"].copy()
    c["wt"][row] = 0.0
    _, score0 = _run(c)
    assert np.all(np.isnan(score0[:3])) and np.all(np.isfinite(score0[3:]))


# ---- the search against the reference fixture --------------------------------

def _selectors():
    from pyabc_amd.transition import scott_rule_of_thumb, silverman_rule_of_thumb
    return {"silverman": silverman_rule_of_thumb, "scott": scott_rule_of_thumb}


def _search(z, c, **kw):
    from pyabc_amd.transition import GridSearchCV
    sel = _selectors()
    scal, names = z[f"{c}__scaling"], [str(n) for n in z[f"{c}__selector"]]
    if len(set(names)) > 1:
        grid = {"scaling": list(dict.fromkeys(scal.tolist())),
                "bandwidth_selector": [sel[n] for n in dict.fromkeys(names)]}
    else:
        grid = {"scaling": scal}
    return GridSearchCV(param_grid=grid, cv=int(z[f"{c}__cv"]), **kw), grid


def _frame(X):
    return pd.DataFrame(X, columns=[f"p{k}" for k in range(X.shape[1])])


def _check_against_fixture(gs, z, c):
    X, w = z[f"{c}__X"], z[f"{c}__w"]
    r = gs.cv_results_
    want_test, want_train = z[f"{c}__test"], z[f"{c}__train"]
    nc, k = want_test.shape
    assert gs.n_splits_ == k and gs.route_ == "device"
    sel = _selectors()
    assert [p["scaling"] for p in r["params"]] == z[f"{c}__scaling"].tolist()
    assert np.array_equal(np.asarray(r["param_scaling"], dtype=float), z[f"{c}__scaling"])
    for p, name in zip(r["params"], z[f"{c}__selector"]):
        assert p.get("bandwidth_selector", sel["silverman"]) is sel[str(name)]
    tol_f = np.array([TOL * w[te].sum() for _, te in ref.kfold(len(X), k)])
    worst = 0.0
    for f in range(k):
        got, want = r[f"split{f}_test_score"], want_test[:, f]
        fin = np.isfinite(want)
        assert np.array_equal(got[~fin], want[~fin]), (c, f)        # -inf
        tol = 1e-7 if (c == "Aiso" and f == k - 1) else tol_f[f]
        err = np.abs(got[fin] - want[fin]).max() if fin.any() else 0.0
        worst = max(worst, err)
        assert err <= tol, (c, f, err, tol)
        got, want = r[f"split{f}_train_score"], want_train[:, f]
        fin = np.isfinite(want)
        assert np.array_equal(got[~fin], want[~fin]), (c, f)
        assert np.abs(got[fin] - want[fin]).max() <= TOL, (c, f)
    print(f"case {c}: max |split test score - reference| = {worst:.3e} "
          f"(bound {tol_f.min():.3e})")
    # means and stds move by no more than the scores do
    for kind, tol in (("test", tol_f.max()), ("train", TOL)):
        for stat in ("mean", "std"):
            got, want = r[f"{stat}_{kind}_score"], z[f"{c}__{stat}_{kind}"]
            fin = np.isfinite(want)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (c, stat, kind)
            assert np.array_equal(got[want == -np.inf], want[want == -np.inf])
            assert np.abs(got[fin] - want[fin]).max() <= tol, (c, stat, kind)
    assert np.array_equal(r["rank_test_score"], z[f"{c}__rank_test"])
    best = int(z[f"{c}__best_index"])
    assert gs.best_index_ == best
    assert gs.best_params_ == r["params"][best]
    assert gs.best_params_["scaling"] == z[f"{c}__scaling"][best]
    assert gs.best_score_ == r["mean_test_score"][best]
    cov, want = np.atleast_2d(gs.best_estimator_.cov), z[f"{c}__cov"]
    assert np.abs(cov - want).max() <= 1e-12 * np.abs(want).max(), c
    assert gs.best_estimator_.scaling == gs.best_params_["scaling"]
    assert not {"mean_fit_time", "mean_score_time"} & set(r)


@pytest.mark.parametrize("c", ["A", "Aiso", "B", "C", "D", "E", "F", "G", "H3"])
def test_fit_against_reference_fixture(golden, c):
    gs, _ = _search(golden, c)
    w = golden[f"{c}__w"].copy()
    with np.errstate(invalid="ignore"):
        gs.fit(_frame(golden[f"{c}__X"]), w)
    _check_against_fixture(gs, golden, c)
    if c == "H3":
        assert gs.cv == 5 and gs.n_splits_ == 3       # reduced for that call only
    if c == "F":
        assert gs.cv_results_["split0_test_score"][0] == -np.inf
    if c == "C":
        assert len(gs.cv_results_["params"]) > CAP    # more than one launch
    if c == "G":
        assert len({p["bandwidth_selector"] for p in gs.cv_results_["params"]}) == 2
    # the fitted search is a transition
    x = _frame(golden[f"{c}__X"][:2])
    assert np.all(np.isfinite(gs.pdf(x))) and gs.rvs(3).shape == (3, x.shape[1])


def test_fit_device_against_reference_fixture(golden):
    gs, _ = _search(golden, "A")
    X = golden["A__X"]
    gs.fit_device(_dev(X), _dev(golden["A__w"]), [f"p{k}" for k in range(X.shape[1])])
    _check_against_fixture(gs, golden, "A")
    assert list(gs.X.columns) == ["p0", "p1", "p2"]
    lp = gs.logpdf_device(_dev(X[:5])).cpu().numpy()
    assert np.all(np.isfinite(lp))
    assert set(gs.proposal_arrays()) >= {"X", "cdf", "L"}


def test_single_particle_fits_the_estimator_directly(golden):
    from pyabc_amd.transition import GridSearchCV
    gs = GridSearchCV()
    gs.fit(_frame(golden["H1__X"]), golden["H1__w"].copy())
    assert gs.best_estimator_ is gs.estimator
    want = golden["H1__cov"]
    assert np.abs(gs.cov - want).max() <= 1e-12 * np.abs(want).max()
    gs = GridSearchCV()
    gs.fit(pd.DataFrame(index=range(4)), np.full(4, 0.25))     # no columns
    assert gs.best_estimator_ is gs.estimator and gs.no_parameters


# ---- routes ------------------------------------------------------------------

def _generic(gs, X, w):
    with np.errstate(invalid="ignore", divide="ignore"):
        gs._fit_generic(_frame(X), w.copy(), None)
    assert gs.route_ == "generic"
    return gs


def _same_search(dev, gen, tol):
    rd, rg = dev.cv_results_, gen.cv_results_
    assert rd["params"] == rg["params"]
    for key in rd:
        if key.startswith("split"):
            fin = np.isfinite(rg[key])
            assert np.array_equal(rd[key][~fin], rg[key][~fin], equal_nan=True), key
            assert np.abs(rd[key][fin] - rg[key][fin]).max() <= tol, key
    assert np.array_equal(rd["rank_test_score"], rg["rank_test_score"])
    assert dev.best_index_ == gen.best_index_ and dev.best_params_ == gen.best_params_
    assert {"mean_fit_time", "std_score_time"} <= set(rg)


@pytest.mark.parametrize("c", ["A", "G"])
def test_device_route_equals_generic_route(golden, c):
    X, w = golden[f"{c}__X"], golden[f"{c}__w"]
    dev, _ = _search(golden, c)
    dev.fit(_frame(X), w.copy())
    assert dev.route_ == "device"
    gen, _ = _search(golden, c)
    _generic(gen, X, w)
    _same_search(dev, gen, 4e-6)             # both sides carry 2e-6
    assert np.abs(dev.best_estimator_.cov - gen.best_estimator_.cov).max() <= \
        1e-12 * np.abs(gen.best_estimator_.cov).max()


def test_singular_covariance_goes_through_the_fallback(golden):
    """A duplicated column: every fold's covariance has rank 2 of 3.  The
    device route answers through the estimator's own fit and direct kernel
    (support mask), as the generic route does."""
    from pyabc_amd.transition import GridSearchCV
    X = golden["A__X"].copy()
    X[:, 2] = X[:, 0]
    w = golden["A__w"]
    dev = GridSearchCV()
    dev.fit(_frame(X), w.copy())
    assert dev.route_ == "device"
    gen = _generic(GridSearchCV(), X, w)
    assert np.all(np.isfinite(gen.cv_results_["mean_test_score"]))
    _same_search(dev, gen, 4e-6)
    assert np.linalg.matrix_rank(dev.best_estimator_.cov) == 2


def test_local_transition_runs_generically():
    """(LocalTransition.k is a read-only property, in the reference too: the
    grid varies k_fraction.)"""
    from pyabc_amd.transition import GridSearchCV, LocalTransition
    X, w = _population(3, 90, 2)
    gs = GridSearchCV(LocalTransition(), {"k_fraction": [0.2, 0.4], "scaling": [0.5, 1.0]},
                      cv=3)
    gs.fit(_frame(X), w)
    assert gs.route_ == "generic" and len(gs.cv_results_["params"]) == 4
    assert isinstance(gs.best_estimator_, LocalTransition)
    assert gs.best_estimator_.k_fraction == gs.best_params_["k_fraction"]
    assert np.all(np.isfinite(gs.pdf(_frame(X[:4])))) and gs.rvs(2).shape == (2, 2)


# ---- ABCSMC ------------------------------------------------------------------

def test_abcsmc_with_gridsearch_stays_on_the_device_loop(caplog):
    """d = 2 conjugate Gaussian model, population 500, 3 generations: the
    posterior per coordinate is N(y / 1.25, 0.2) as eps -> 0; thresholds of
    test_gpu_e2e.py (mean 0.07, sd 0.12)."""
    import pyabc_amd as pa
    np.random.seed(0)
    model = pa.LinearGaussianModel(["x0", "x1"], ["y0", "y1"], src=[0, 1],
                                   sigma=[0.5, 0.5])
    prior = pa.Distribution(x0=pa.RV("norm", 0, 1), x1=pa.RV("norm", 0, 1))
    tr = pa.GridSearchCV()
    abc = pa.ABCSMC(model, prior, pa.PNormDistance(), population_size=500,
                    sampler=pa.BatchedGPUSampler(seed=1000, allow_per_candidate=False),
                    transitions=tr, eps=pa.MedianEpsilon(.2))
    abc.new("sqlite://", {"y0": 2.0, "y1": -1.0})
    fitted = []
    orig = tr.fit_device

    def spy(*a, **k):
        res = orig(*a, **k)
        fitted.append((tr.route_, dict(tr.best_params_)))
        return res
    tr.fit_device = spy
    with caplog.at_level(logging.WARNING):
        h = abc.run(minimum_epsilon=-1, max_nr_populations=3)
    assert h.max_t == 2
    spec = pa.GenerationSpec(abc, 1)
    assert spec.batched_capable and spec.why_not == ""
    assert not [r for r in caplog.records
                if "per-candidate" in r.getMessage() or "no device kernel" in r.getMessage()]
    # fitted before generations 1 and 2 (and after the last), on the device
    assert len(fitted) >= 2 and all(route == "device" for route, _ in fitted)
    assert all(p["scaling"] in np.linspace(0.05, 1.0, 5) for _, p in fitted)
    df, w = h.get_distribution(0, h.max_t)
    for name, y in (("x0", 2.0), ("x1", -1.0)):
        x = df[name].values
        mean = float((x * w).sum())
        sd = float(np.sqrt((w * (x - mean) ** 2).sum()))
        assert abs(mean - y / 1.25) < 0.07, (name, mean)
        assert abs(sd - np.sqrt(0.2)) < 0.12, (name, sd)
