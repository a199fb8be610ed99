"""pyabc_amd.visualization on the device: abc_kde_panels against the float64
restatement (tests/kde_ref.py) and the pyABC 0.10.5 fixture
(tests/golden/kde.npz, made by make_golden_kde.py), the routes, the credible
functions and the plot functions.

Tolerances.  2e-6 absolute per log density, the project's contract for its
fp64 density kernels (fp64 differences and exponent, fp32 exp2), at every grid
point whose reference density is >= 1e-290; below that the device density is
only bounded (< 1e-289).  2e-6 relative against the golden densities >= 1e-280.
Measured maxima are in DESIGN.md section 7e.
"""
import os

import matplotlib
matplotlib.use("Agg")

import numpy as np
import pandas as pd
import pytest

import kde_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 2e-6
LOG_FLOOR = float(np.log(1e-290))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "kde.npz"))


def _frame(X, names=None):
    return pd.DataFrame(X, columns=names or [f"p{k}" for k in range(X.shape[1])])


def _population(seed, N, d, zero=False):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(d, d)) + 2 * np.eye(d)
    X = rng.normal(size=(N, d)) @ A.T + rng.normal(size=d)
    w = rng.gamma(1.0, size=N)
    if zero and N > 4:
        w[rng.permutation(N)[:N // 4]] = 0.0
    return X, w / w.sum()


def _kde_of(case):
    import pyabc_amd as pa
    from pyabc_amd.transition.multivariatenormal import (scott_rule_of_thumb,
                                                         silverman_rule_of_thumb)
    if case["scaling"] == 1.0 and case["rule"] == "silverman":
        return None
    rule = {"scott": scott_rule_of_thumb, "silverman": silverman_rule_of_thumb}[case["rule"]]
    return pa.MultivariateNormalTransition(scaling=case["scaling"], bandwidth_selector=rule)


def _device_panels(case):
    """{key: density array} of a case's panels through the public functions:
    kde_matrix when the case holds the whole matrix, else kde_1d / kde_2d."""
    from pyabc_amd import visualization as vis
    df, w = _frame(case["X"]), case["w"].copy()
    lim = case["limits"]
    if case["keys"] == ref.matrix_keys(case["names"]):
        res = vis.kde_matrix(df, w, lim, case["numx"], case["numy"], _kde_of(case))
        assert res.route_ == "device"
        return {k: v[-1] for k, v in res.items()}, res.panel_routes_
    out = {}
    for key in case["keys"]:
        lims = [lim.get(n, (None, None)) for n in key]
        if len(key) == 1:
            out[key] = vis.kde_1d(df, w, key[0], lims[0][0], lims[0][1], case["numx"],
                                  _kde_of(case))[1]
        else:
            out[key] = vis.kde_2d(df, w, key[0], key[1], lims[0][0], lims[0][1],
                                  lims[1][0], lims[1][1], case["numx"], case["numy"],
                                  _kde_of(case))[2]
    return out, None


def _check_against_ref(dens, lp_ref, tag):
    dens = np.asarray(dens, dtype=np.float64).reshape(lp_ref.shape)
    live = lp_ref >= LOG_FLOOR
    with np.errstate(divide="ignore"):
        err = np.abs(np.log(dens[live]) - lp_ref[live])
    worst = float(err.max()) if err.size else 0.0
    print(f"{tag}: max |log dev - ref| = {worst:.3e} over {int(live.sum())} points, "
          f"{int((~live).sum())} below the floor")
    assert worst <= TOL, (tag, worst)
    assert np.all(dens[~live] < 1e-289), tag


@pytest.mark.parametrize("c", ref.GOLDEN_CASES)
def test_golden_cases(golden, c):
    case = ref.golden_case(golden, c)
    dens, routes = _device_panels(case)
    for key in case["keys"]:
        gold = case["pdf"][key]
        got = np.asarray(dens[key], dtype=np.float64).reshape(gold.shape)
        _check_against_ref(got, ref.log_panel(case, key).reshape(gold.shape), f"{c} {key}")
        big = gold >= 1e-280
        rel = np.abs(got[big] - gold[big]) / gold[big]
        print(f"{c} {key}: max rel to golden {rel.max() if rel.size else 0:.3e}")
        assert np.all(rel <= TOL), (c, key, rel.max())
    if routes is not None:
        # D's pair: variances 1e-6 and 1e8 are further apart than scipy's
        # eigenvalue cut (1e6 eps), so the reference itself fits it as singular
        irregular = {"D": {("p0", "p1")}, "I": set(case["keys"])}.get(c, set())
        assert {k for k, v in routes.items() if v == "estimator"} == irregular


SHAPES = [  # N, d, numx, numy, zero weights
    (1, 2, 7, 13, False), (2, 2, 7, 13, False), (255, 1, 64, 1, False),
    (256, 2, 50, 50, True), (257, 7, 50, 50, False), (257, 2, 1, 1, False),
    (4099, 2, 50, 50, True), (4099, 7, 7, 13, False), (100003, 2, 7, 13, True),
    (100003, 1, 1, 1, False), (100003, 1, 64, 1, False)]


@pytest.mark.parametrize("N,d,numx,numy,zero", SHAPES)
def test_shapes_against_restatement(N, d, numx, numy, zero):
    from pyabc_amd import visualization as vis
    X, w = _population(100 + N + d, N, d, zero)
    names = [f"p{k}" for k in range(d)]
    # limits for every second parameter, reaching past the sample
    limits = {names[k]: (X[:, k].min() - 1.0, None) for k in range(0, d, 2)}
    res = vis.kde_matrix(_frame(X), w.copy(), limits, numx, numy)
    assert res.route_ == "device" and len(res) == d * (d + 1) // 2
    lp = ref.log_kde_matrix(X, w, names, limits, numx, numy)
    for key, val in res.items():
        assert val[-1].shape == ((numx,) if len(key) == 1 else (numy, numx))
        _check_against_ref(val[-1], lp[key], f"N={N} d={d} {numx}x{numy} {key}")
        expect = "estimator" if (N == 1 or (N == 2 and len(key) == 2)) else "kernel"
        assert res.panel_routes_[key] == expect
        ax = ref.axes(X, names, key, limits, numx, numy)
        assert np.array_equal(val[0] if len(key) == 1 else val[0][0], ax[0])
        if len(key) == 2:
            assert np.array_equal(val[1][:, 0], ax[1])


def test_partial_budget_plan_on_a_large_grid():
    """More grid points than the partial-pair budget holds at 64 chunks
    (64 G_total > 2^22): the chunk count comes from the budget.  The
    restatement is evaluated at a sample of the 66 563 grid points."""
    from pyabc_amd import visualization as vis
    N, n = 70001, 257
    X, w = _population(77, N, 2, True)
    names = ["p0", "p1"]
    res = vis.kde_matrix(_frame(X), w.copy(), None, n, n)
    assert set(res.panel_routes_.values()) == {"kernel"}
    Xg, Yg, PDF = res[("p0", "p1")]
    rng = np.random.default_rng(0)
    pick = rng.choice(n * n, size=300, replace=False)
    pick[:4] = [0, n - 1, n * n - n, n * n - 1]            # the corners
    pts = np.stack([Xg.ravel()[pick], Yg.ravel()[pick]], axis=1)
    lp = ref.log_kde(pts, X, w, ref.fit_cov(X, w))
    _check_against_ref(PDF.ravel()[pick], lp, "budget 2-D")
    x, pdf = res[("p1",)]
    pick = np.arange(0, n, 7)
    lp = ref.log_kde(x[pick, None], X[:, [1]], w, ref.fit_cov(X[:, [1]], w))
    _check_against_ref(pdf[pick], lp, "budget 1-D")


def test_far_offset_and_wide_limits_stay_within_tolerance():
    """The population far from the origin (1e8) at unit scale: centring comes
    before squaring."""
    from pyabc_amd import visualization as vis
    X, w = _population(9, 300, 2)
    names = ["p0", "p1"]
    # unit scale at 1e8; scales 1e-3 and 10 at 1e6 (variances 1e8 apart: inside
    # scipy's eigenvalue cut, so the pair is a kernel panel)
    for tag, Y in (("1e8", X + 1e8), ("scales", X * np.array([1e-3, 10.0]) + 1e6)):
        res = vis.kde_matrix(_frame(Y), w.copy(), None, 20, 20)
        assert set(res.panel_routes_.values()) == {"kernel"}
        lp = ref.log_kde_matrix(Y, w, names, None, 20, 20)
        for key, val in res.items():
            _check_against_ref(val[-1], lp[key], f"offset {tag} {key}")


def test_panel_independence_and_repeat(golden):
    from pyabc_amd import visualization as vis
    case = ref.golden_case(golden, "B")
    df, w = _frame(case["X"]), case["w"]
    lim = case["limits"]
    res = vis.kde_matrix(df, w.copy(), lim, 50, 50)
    again = vis.kde_matrix(df, w.copy(), lim, 50, 50)
    for key in res:
        assert np.array_equal(res[key][-1], again[key][-1]), key       # bitwise
    for key in (("p0", "p1"), ("p1", "p2")):
        lx, ly = lim.get(key[0], (None, None)), lim.get(key[1], (None, None))
        Xg, Yg, PDF = vis.kde_2d(df, w.copy(), key[0], key[1], lx[0], lx[1], ly[0], ly[1])
        assert np.array_equal(Xg, res[key][0]) and np.array_equal(Yg, res[key][1])
        assert np.allclose(PDF, res[key][2], rtol=1e-12, atol=0), key
    x, pdf = vis.kde_1d(df, w.copy(), "p2")
    assert np.allclose(pdf, res[("p2",)][1], rtol=1e-12, atol=0)
    # a non-square matrix whose panels end inside a tile: 7 x 13 = 91 points
    small = vis.kde_matrix(df, w.copy(), lim, 7, 13)
    one = vis.kde_2d(df, w.copy(), "p0", "p2", None, None, None, None, 7, 13)
    assert np.allclose(one[2], small[("p0", "p2")][2], rtol=1e-12, atol=0)


@pytest.mark.parametrize("c", ["H", "I"])
def test_irregular_panels_are_the_estimators_own(golden, c):
    import pyabc_amd as pa
    from pyabc_amd import visualization as vis
    case = ref.golden_case(golden, c)
    df = _frame(case["X"])
    lim = case["limits"]
    for key in case["keys"]:
        lims = [lim.get(n, (None, None)) for n in key]
        est = pa.MultivariateNormalTransition(scaling=1)
        est.fit(df[list(key)], case["w"].copy())
        axes = ref.axes(case["X"], case["names"], key, lim, case["numx"], case["numy"])
        if len(key) == 1:
            own = est.pdf(pd.DataFrame({key[0]: axes[0]}))
            got = vis.kde_1d(df, case["w"].copy(), key[0], lims[0][0], lims[0][1],
                             case["numx"])[1]
        else:
            Xg, Yg = np.meshgrid(*axes)
            own = est.pdf(pd.DataFrame({key[0]: Xg.flatten(), key[1]: Yg.flatten()}))
            got = vis.kde_2d(df, case["w"].copy(), key[0], key[1], lims[0][0], lims[0][1],
                             lims[1][0], lims[1][1], case["numx"], case["numy"])[2]
        assert np.array_equal(np.asarray(own).reshape(got.shape), got), (c, key)


def test_generic_route_with_local_transition():
    import pyabc_amd as pa
    from pyabc_amd import visualization as vis
    X, w = _population(4, 200, 2)
    df = _frame(X)
    kde = pa.LocalTransition()
    res = vis.kde_matrix(df, w.copy(), None, 9, 11, kde)
    assert res.route_ == "generic"
    assert set(res.panel_routes_.values()) == {"estimator"}
    for key, val in res.items():
        est = pa.LocalTransition()
        est.fit(df[list(key)], w.copy())
        axes = ref.axes(X, ["p0", "p1"], key, None, 9, 11)
        if len(key) == 1:
            own = est.pdf(pd.DataFrame({key[0]: axes[0]}))
        else:
            Xg, Yg = np.meshgrid(*axes)
            own = est.pdf(pd.DataFrame({key[0]: Xg.flatten(), key[1]: Yg.flatten()}))
        assert np.allclose(np.asarray(own).reshape(val[-1].shape), val[-1], rtol=1e-12)
    # the device route leaves the passed estimator unfitted
    mvn = pa.MultivariateNormalTransition(scaling=0.5)
    assert vis.kde_matrix(df, w.copy(), None, 9, 11, mvn).route_ == "device"
    assert mvn.cov is None and mvn._X_arr is None and "X" not in mvn.__dict__


def test_quantiles_and_credible_intervals(golden):
    from pyabc_amd import visualization as vis
    from pyabc_amd.weighted_statistics import weighted_quantile
    X, w = golden["B__X"], golden["B__w"]
    for k in range(3):
        assert vis.compute_quantile(X[:, k], w, 0.5) == pytest.approx(
            golden["B__median"][k], rel=1e-12)
        for j, level in enumerate((0.5, 0.95)):
            got = vis.compute_credible_interval(X[:, k], w, level)
            assert np.allclose(got, golden["B__ci"][k, j], rtol=1e-12, atol=0)
    # ties and a run of zero weights
    rng = np.random.default_rng(1)
    v = np.round(rng.normal(size=3000), 1)                 # ~60 distinct values
    ww = rng.gamma(1.0, size=3000)
    ww[1000:1400] = 0.0
    ww /= ww.sum()
    for alpha in (0.025, 0.25, 0.5, 0.75, 0.975):
        host = weighted_quantile(v, ww, alpha=alpha)
        assert vis.compute_quantile(v, ww, alpha) == pytest.approx(host, rel=1e-12, abs=1e-300)
    lb, ub = vis.compute_credible_interval(v, ww, 0.95)
    assert lb == pytest.approx(weighted_quantile(v, ww, alpha=0.025), rel=1e-12)
    assert ub == pytest.approx(weighted_quantile(v, ww, alpha=0.975), rel=1e-12)
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            vis.compute_credible_interval(v, ww, bad)


def test_kde_max_index(golden):
    import pyabc_amd as pa
    from pyabc_amd import visualization as vis
    X, w = golden["K__X"], golden["K__w"]
    df = _frame(X)
    ix, _ = vis.kde_max_index(pa.MultivariateNormalTransition(), df, w.copy())
    assert ix == int(golden["K__kde_max_index"])
    pnt = vis.compute_kde_max(pa.MultivariateNormalTransition(), df, w.copy())
    assert list(pnt.index) == ["p0", "p1"] and np.array_equal(pnt.values, X[ix])
    # the lowest index among equal maxima: every particle twice, so whichever
    # is the largest ties with its copy N rows on
    X2, w2 = np.concatenate([X, X], axis=0), np.concatenate([w, w]) / 2
    assert vis.kde_max_index(pa.MultivariateNormalTransition(), _frame(X2), w2)[0] < len(X)


# ---- plots ---------------------------------------------------------------------

def test_plot_functions(golden):
    import matplotlib.pyplot as plt
    from matplotlib.collections import PathCollection, QuadMesh
    from pyabc_amd import visualization as vis
    case = ref.golden_case(golden, "B")
    df, w = _frame(case["X"]), case["w"]
    lim = case["limits"]
    refval = {"p0": 0.1, "p1": 0.2, "p2": 0.3}
    res = vis.kde_matrix(df, w.copy(), lim, 20, 15)
    arr = vis.plot_kde_matrix(df, w.copy(), lim, numx=20, numy=15, refval=refval,
                              scatter_max=100)
    assert arr.shape == (3, 3)
    names = list(df.columns)
    for i, yn in enumerate(names):
        line = arr[i, i].get_lines()[0]
        assert np.array_equal(line.get_xdata(), res[(yn,)][0])
        assert np.array_equal(line.get_ydata(), res[(yn,)][1])
        for j in range(i):
            mesh = [c for c in arr[i, j].collections if isinstance(c, QuadMesh)][0]
            assert np.array_equal(np.asarray(mesh.get_array()).reshape(15, 20),
                                  res[(names[j], yn)][2])
            pts = [c for c in arr[j, i].collections if isinstance(c, PathCollection)][0]
            assert len(pts.get_offsets()) == 100                   # thinned from 1000
    assert arr[2, 0].get_xlabel() == "p0" and arr[1, 0].get_ylabel() == "p1"
    assert arr[0, 1].get_xlabel() == "" and arr[1, 1].get_ylabel() == ""
    full = vis.plot_kde_matrix(df, w.copy(), numx=5, numy=5, colorbar=False)
    pts = [c for c in full[0, 1].collections if isinstance(c, PathCollection)][0]
    assert len(pts.get_offsets()) == 1000
    ax = vis.plot_kde_1d(df, w.copy(), "p0", numx=20, refval=refval, title="t")
    assert ax.get_xlabel() == "p0" and ax.get_ylabel() == "Posterior"
    assert len(ax.get_lines()) == 2 and ax.get_title() == "t"
    ax = vis.plot_kde_2d(df, w.copy(), "p0", "p1", numx=20, numy=15, refval=refval)
    assert ax.get_xlabel() == "p0" and ax.get_ylabel() == "p1"
    assert len(ax.get_figure().axes) == 2                          # the colour bar
    plt.close("all")


def _run(models, priors, **kw):
    import pyabc_amd as pa
    np.random.seed(0)
    abc = pa.ABCSMC(models, priors, pa.PNormDistance(), population_size=500,
                    sampler=pa.BatchedGPUSampler(seed=1000, allow_per_candidate=False),
                    eps=pa.MedianEpsilon(.5), **kw)
    abc.new("sqlite://", {"y0": 1.0, "y1": 0.6})
    return abc.run(minimum_epsilon=-1, max_nr_populations=2)


def _check_highlevel(h, m, names):
    import matplotlib.pyplot as plt
    from pyabc_amd import visualization as vis
    assert h.get_population_device(h.max_t, m) is not None           # resident
    df, w = h.get_distribution(m=m, t=h.max_t)
    assert list(df.columns) == names
    arr = vis.plot_kde_matrix_highlevel(h, m=m, numx=12, numy=10)
    assert arr.shape == (len(names),) * 2
    # against the same population through the host frame: the weights differ
    # in their last bit (normalised there and here), which moves single fp32
    # exp2 roundings: both sides are within TOL of the exact density
    host = vis.kde_matrix(df, w.copy(), None, 12, 10)
    for i, n in enumerate(names):
        line = arr[i, i].get_lines()[0]
        assert np.allclose(line.get_ydata(), host[(n,)][1], rtol=2 * TOL)
    ax = vis.plot_kde_1d_highlevel(h, names[0], m=m, numx=12)
    assert np.allclose(ax.get_lines()[0].get_ydata(), host[(names[0],)][1], rtol=2 * TOL)
    if len(names) > 1:
        ax = vis.plot_kde_2d_highlevel(h, names[0], names[1], m=m, numx=12, numy=10)
        assert ax.get_xlabel() == names[0] and ax.get_ylabel() == names[1]
    axs = vis.plot_credible_intervals(h, m=m, levels=[0.5, 0.95], show_mean=True,
                                      show_kde_max=True, show_kde_max_1d=True)
    assert len(axs) == len(names)
    for n, ax in zip(names, axs):
        assert ax.get_title() == f"Parameter {n}" and ax.get_ylabel() == n
        labels = ax.get_legend_handles_labels()[1]
        assert set(labels) == {"0.50", "0.95", "Mean", "Max KDE", "Max KDE 1d"}
    # the medians drawn are the host quantiles
    from pyabc_amd.weighted_statistics import weighted_quantile
    med = weighted_quantile(np.asarray(df[names[0]]), w, alpha=0.5)
    drawn = [ln for ln in axs[0].get_lines() if len(ln.get_ydata()) == h.max_t + 1]
    assert any(abs(ln.get_ydata()[-1] - med) <= 1e-9 * max(1, abs(med)) for ln in drawn)
    plt.close("all")


def test_highlevel_from_a_batched_run_one_model():
    import pyabc_amd as pa
    model = pa.LinearGaussianModel(["x0", "x1"], ["y0", "y1"], src=[0, 1],
                                   sigma=[0.5, 0.5])
    prior = pa.Distribution(x0=pa.RV("norm", 0, 1), x1=pa.RV("norm", 0, 1))
    h = _run(model, prior)
    assert h.max_t == 1
    _check_highlevel(h, 0, ["x0", "x1"])
    # a model the run does not have: no particles, as the reference's
    # get_distribution(m=1) gives (not model 0's resident columns)
    from pyabc_amd import visualization as vis
    with pytest.raises(pa.NotEnoughParticles):
        vis.plot_kde_1d_highlevel(h, "x0", m=1)
    with pytest.raises(pa.NotEnoughParticles):
        vis.plot_kde_matrix_highlevel(h, m=1)
    # the numbers behind the credible plot, per generation
    tab = vis.interval_table(h, 0, [0, 1], ["x1"], [0.5, 0.95], mean=True)
    assert set(tab) == {"x1"} and tab["x1"]["lower"].shape == (2, 2)
    df, w = h.get_distribution(m=0, t=1)
    v = np.asarray(df["x1"])
    assert np.allclose([tab["x1"]["lower"][1, 1], tab["x1"]["upper"][1, 1]],
                       ref.credible_interval(v, w, 0.95), rtol=1e-9)
    assert tab["x1"]["mean"][1] == pytest.approx(float(np.sum(v * w)), rel=1e-9)
    assert np.all(tab["x1"]["lower"][1] <= tab["x1"]["lower"][0])
    assert np.all(tab["x1"]["upper"][1] >= tab["x1"]["upper"][0])


def test_highlevel_from_a_batched_run_two_models():
    import pyabc_amd as pa
    A = pa.LinearGaussianModel(["a"], ["y0", "y1"], [0, 0], sigma=[0.5] * 2, name="A")
    B = pa.LinearGaussianModel(["b0", "b1"], ["y0", "y1"], [0, 1], sigma=[0.5] * 2, name="B")
    priors = [pa.Distribution(a=pa.RV("uniform", 0.7, 2.0)),
              pa.Distribution(b0=pa.RV("norm", 0.5, 1.0), b1=pa.RV("norm", 0.5, 1.0))]
    h = _run([A, B], priors,
             model_prior=pa.RV("rv_discrete", values=([0, 1], [0.25, 0.75])),
             model_perturbation_kernel=pa.ModelPerturbationKernel(2, 0.9))
    assert h.max_t == 1
    _check_highlevel(h, 1, ["b0", "b1"])
