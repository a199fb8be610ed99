"""The KDE-panel reference, the host planner and the entry's host side (no
device): tests/kde_ref.py against the golden vectors of the pyABC reference,
plan_panels against the golden fits, the workspace query and the argument
checks of abc_kde_panels, and the conditions the GPU tests rely on, checked
here on the fixture by the reference alone."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import kde_ref as ref


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "kde.npz"))


@pytest.mark.parametrize("c", ref.GOLDEN_CASES)
def test_reference_restatement_matches_golden(golden, c):
    case = ref.golden_case(golden, c)
    for key in case["keys"]:
        gold = case["pdf"][key]
        with np.errstate(over="ignore"):
            mine = np.exp(ref.log_panel(case, key)).reshape(gold.shape)
        big = gold >= 1e-280
        assert np.allclose(mine[big], gold[big], rtol=1e-9, atol=0), (c, key)
        # below that the reference's plain sum loses terms to underflow: the
        # restatement is at least as large, and never large where gold is 0
        assert np.all(mine[~big] < 1e-279), (c, key)
        # the axes are the reference's
        axes = ref.axes(case["X"], case["names"], key, case["limits"],
                        case["numx"], case["numy"])
        assert np.array_equal(axes[0], case["x"][key])
        if len(key) == 2:
            assert np.array_equal(axes[1], case["y"][key])


def _plan(case, **kw):
    from pyabc_amd.visualization import plan_panels
    X, w = case["X"], case["w"]
    N = len(X)
    cov = np.atleast_2d(np.cov(X, aweights=w, rowvar=False)) if N > 1 else \
        np.full((X.shape[1],) * 2, np.nan)
    return plan_panels(case["names"], cov, 1 / np.sum(w ** 2), X.min(axis=0),
                       X.max(axis=0), case["limits"], case["numx"], case["numy"],
                       case["scaling"], {"silverman": 0, "scott": 1}[case["rule"]],
                       case["keys"], mean=np.average(X, axis=0, weights=w),
                       n_particles=N, **kw)


@pytest.mark.parametrize("c", [c for c in ref.GOLDEN_CASES if c != "I"])
def test_plan_panels_matches_golden_fits(golden, c):
    case = ref.golden_case(golden, c)
    plan = _plan(case)
    assert [q["key"] for q in plan.panels] == case["keys"]
    off = 0
    for q in plan.panels:
        key, k = q["key"], len(q["key"])
        gold = case["cov"][key]
        # (absolute: a constant column's moments are the rounding of its
        # weighted mean, up to (4 eps |x|)^2, in the reference's fit too)
        atol = (4 * np.finfo(np.float64).eps * np.abs(case["X"]).max()) ** 2
        assert np.allclose(q["cov"], gold, rtol=1e-10, atol=atol), (c, key)
        assert q["bw"] == pytest.approx(
            ref.bandwidth(case["rule"], 1 / np.sum(case["w"] ** 2), k), rel=1e-14)
        assert np.array_equal(q["axes"][0], case["x"][key])
        if k == 2:
            assert np.array_equal(q["axes"][1], case["y"][key])
        if q["irregular"]:
            continue
        sign, logdet = np.linalg.slogdet(gold)
        assert sign > 0
        assert q["log_const"] == pytest.approx(-0.5 * (k * ref.LOG_2PI + logdet),
                                               rel=1e-9, abs=1e-9)
        # U U^T = cov^-1
        assert np.allclose(q["U"] @ q["U"].T @ gold, np.eye(k), atol=1e-6)
        assert q["out"] == off
        off += q["num"][0] * q["num"][1]
    assert plan.n_points == off
    assert plan.coords.size == sum(a.size for q in plan.regular for a in q["axes"])


def test_irregular_panel_flags(golden):
    H = ref.golden_case(golden, "H")
    flags = {q["key"]: q["irregular"] for q in _plan(H).panels}
    assert flags == {("p1",): True, ("p0", "p1"): True, ("p0", "p2"): True}
    I = ref.golden_case(golden, "I")
    assert all(q["irregular"] for q in _plan(I).panels)
    B = ref.golden_case(golden, "B")
    assert not any(q["irregular"] for q in _plan(B).panels)
    # the 0.999 pair is ill-conditioned, not singular: it goes to the kernel
    C = ref.golden_case(golden, "C")
    assert not any(q["irregular"] for q in _plan(C).panels)
    # D's pair (variances 1e-6 and 1e8) lies beyond scipy's eigenvalue cut: the
    # reference itself fits it as singular; its 1-D panels are regular
    D = ref.golden_case(golden, "D")
    flags = {q["key"]: q["irregular"] for q in _plan(D).panels}
    assert flags == {("p0",): False, ("p0", "p1"): True, ("p1",): False}
    # N == 1 is irregular whatever the covariance handed over
    from pyabc_amd.visualization import plan_panels
    p = plan_panels(["a"], [[1.0]], 1.0, [0.0], [1.0], n_particles=1)
    assert p.panels[0]["irregular"] and p.coords.size == 0


def test_descriptors_mirror_the_plan(golden):
    from pyabc_amd import _native as nat
    plan = _plan(ref.golden_case(golden, "B"))
    desc = plan.descriptors()
    assert ctypes.sizeof(nat.KdePanel) == 96
    assert len(desc) == len(plan.regular) == 6
    for a, q in zip(desc, plan.regular):
        two = len(q["key"]) == 2
        assert (a.col[0], a.col[1]) == (q["cols"][0], q["cols"][1] if two else -1)
        assert (a.num[0], a.num[1]) == q["num"]
        assert a.out == q["out"] and a.log_const == q["log_const"]
        assert [a.U[k] for k in range(q["U"].size)] == list(q["U"].ravel())
        x = plan.coords[a.axis[0]:a.axis[0] + a.num[0]]
        assert np.array_equal(x, q["axes"][0])


def test_bytes_query_is_positive_monotone_and_zero_when_rejected():
    from pyabc_amd import _native as nat

    def q(N, d, P, G):
        return nat.query("abc_kde_panels_bytes", N, d, P, G)
    base = (10 ** 6, 10, 55, 113000)
    assert q(*base) > 0
    grids = dict(N=[1, 2, 255, 256, 257, 1024, 1025, 4099, 65535, 65536, 65537,
                    100003, 10 ** 6, 10 ** 7],
                 d=[1, 2, 7, 10, 64],
                 P=[1, 2, 28, 55, 56, 1000, 2080],
                 G=[1, 50, 2500, 65535, 65536, 65537, 113000, 2 ** 20, 2 ** 22 - 1,
                    2 ** 22, 2 ** 22 + 1, 5 * 10 ** 6, 2 ** 24])
    for i, name in enumerate("NdPG"):
        for other in (base, (257, 2, 3, 2600), (1, 1, 1, 1)):
            vals = []
            for v in grids[name]:
                a = list(other)
                a[i] = v
                vals.append(q(*a))
            assert all(x > 0 for x in vals), (name, vals)
            assert all(x <= y for x, y in zip(vals, vals[1:])), (name, vals)
    for bad in ((0, 10, 55, 113000), (10 ** 6, 0, 55, 113000), (10 ** 6, 65, 55, 113000),
                (10 ** 6, 10, 0, 113000), (10 ** 6, 10, 2081, 113000),
                (10 ** 6, 10, 55, 0), (10 ** 6, 10, 55, 2 ** 24 + 1), (-1, 10, 55, 113000)):
        assert q(*bad) == 0, bad
    # the c3 posterior matrix: partial pairs within the 2^22 budget
    assert q(*base) < 80e6


def _one_panel(**kw):
    from pyabc_amd import _native as nat
    a = (nat.KdePanel * 1)()
    a[0].col[0], a[0].col[1] = kw.get("col", (0, -1))
    a[0].num[0], a[0].num[1] = kw.get("num", (4, 1))
    a[0].axis[0], a[0].axis[1] = kw.get("axis", (0, 0))
    a[0].centre[0] = 0.0
    a[0].U[0] = kw.get("u", 1.0)
    a[0].log_const = 0.0
    a[0].out = kw.get("out", 0)
    return a


def test_argument_errors_without_a_device():
    from pyabc_amd import _native as nat
    fake = ctypes.c_void_p(256)      # never dereferenced: the checks come first

    def call(N=10, d=2, desc=None, P=1, n_coords=4, G=4, X=fake, ws=fake, nb=1 << 20):
        desc = _one_panel() if desc is None else desc
        return nat.call("abc_kde_panels", X, fake, N, d,
                        ctypes.cast(desc, ctypes.c_void_p), P, fake, n_coords, fake, G,
                        ws, nb, None)
    for kw in (dict(N=0), dict(d=0), dict(P=0), dict(G=0), dict(n_coords=0),
               dict(X=None), dict(ws=None),
               dict(desc=_one_panel(col=(2, -1))), dict(desc=_one_panel(col=(0, 5))),
               dict(desc=_one_panel(num=(0, 1))), dict(desc=_one_panel(num=(4, 2)), G=8),
               dict(desc=_one_panel(axis=(1, 0))), dict(desc=_one_panel(axis=(-1, 0))),
               dict(desc=_one_panel(out=3)), dict(desc=_one_panel(u=float("nan"))),
               dict(G=5), dict(G=3)):
        with pytest.raises(ValueError):
            call(**kw)
        assert "kde_panels" in nat.load().abc_last_error().decode()
    for kw in (dict(d=65), dict(P=2081), dict(G=2 ** 24 + 1),
               dict(desc=_one_panel(num=(4097, 1)), G=4097, n_coords=4097)):
        with pytest.raises(nat.NativeError) as e:
            call(**kw)
        assert e.value.code == nat.ABC_ERR_UNSUPPORTED
    with pytest.raises(nat.NativeError) as e:
        call(nb=64)
    assert e.value.code == nat.ABC_ERR_WORKSPACE


def test_route_and_lazy_matplotlib():
    import subprocess
    out = subprocess.run(
        [sys.executable, "-c",
         "import sys, pyabc_amd as pyabc; v = pyabc.visualization; "
         "v.plot_kde_matrix_highlevel, v.plot_credible_intervals, v.kde_matrix; "
         "print('matplotlib' in sys.modules)"],
        capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().endswith("False")
    import pyabc_amd as pyabc
    v = pyabc.visualization
    T = pyabc.MultivariateNormalTransition
    assert v.route(None) == "device"
    assert v.route(T(scaling=0.3)) == "device"
    from pyabc_amd.transition.multivariatenormal import scott_rule_of_thumb
    assert v.route(T(bandwidth_selector=scott_rule_of_thumb)) == "device"
    assert v.route(T(bandwidth_selector=lambda n, d: 0.5)) == "generic"
    assert v.route(pyabc.LocalTransition()) == "generic"
    assert v.route(None, d=65) == "generic"
    assert v.route(None, numx=4097) == "generic"
    assert v.route(None, d=10, n_panels=55, n_points=2 ** 24 + 1) == "generic"
    # a frame without weights is refused by name, before any device is asked for
    import pandas as pd
    with pytest.raises(ValueError, match="weights"):
        v.kde_matrix(pd.DataFrame({"a": [0.0, 1.0]}))
    assert v.matrix_pairs(["a", "b", "c"]) == [("a",), ("b",), ("a", "b"), ("c",),
                                                ("a", "c"), ("b", "c")]
    with pytest.raises(ValueError):
        v.compute_credible_interval(np.zeros(3), np.ones(3) / 3, 1.0)
    with pytest.raises(ValueError):
        v.compute_credible_interval(np.zeros(3), np.ones(3) / 3, 0.0)


def test_fixture_conditions_hold_by_the_reference_alone(golden):
    """What tests/test_gpu_kde.py assumes about the fixture."""
    # the MAP index: the top two reference densities are well apart
    vals = golden["K__kde_vals"]
    top = np.sort(vals)[::-1]
    assert (top[0] - top[1]) / top[0] > 1e-5
    assert int(np.argmax(vals)) == int(golden["K__kde_max_index"])
    ix, lp = ref.kde_max_index(golden["K__X"], golden["K__w"])
    assert ix == int(golden["K__kde_max_index"])
    assert np.allclose(np.exp(lp), vals, rtol=1e-9)
    # G reaches densities that are exactly 0 in the reference, and the
    # restated log density is finite there (the device is only bounded below
    # 1e-290, not compared)
    G = ref.golden_case(golden, "G")
    for key in G["keys"]:
        gold = G["pdf"][key]
        assert np.any(gold == 0.0) and np.any(gold > 1e-3)
        assert np.all(np.isfinite(ref.log_panel(G, key)))
    # a quarter of E's weights are 0; C's correlation; D's scales and offset
    assert np.sum(golden["E__w"] == 0) == 100
    assert np.corrcoef(golden["C__X"].T)[0, 1] > 0.998
    D = golden["D__X"]
    assert np.all(np.abs(D.mean(axis=0) - 1e6) < 1e3)
    assert 5e-4 < D[:, 0].std() < 2e-3 and 5e3 < D[:, 1].std() < 2e4
    # the credible bounds: restated quantiles equal the reference's
    X, w = golden["B__X"], golden["B__w"]
    for k in range(3):
        assert ref.quantile(X[:, k], w, 0.5) == pytest.approx(golden["B__median"][k], rel=1e-13)
        for j, level in enumerate((0.5, 0.95)):
            assert np.allclose(ref.credible_interval(X[:, k], w, level), golden["B__ci"][k, j],
                               rtol=1e-13)
    # singular and N = 1 panels: the reference's values exist and are finite
    for c in ("H", "I"):
        case = ref.golden_case(golden, c)
        for key in case["keys"]:
            assert np.all(np.isfinite(case["pdf"][key])), (c, key)
