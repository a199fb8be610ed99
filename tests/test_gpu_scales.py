"""abc_column_scale: the ten sum-stat scale functions of
pyabc/distance/scale.py:38-135 per column of a device [R x S] matrix, against
the reference's own formulas evaluated in numpy here and against the
reference's values in tests/golden/scales.npz.

Tolerances.  The median kinds (MAD, MAD_TO_OBS, CMAD) are exact order
statistics of fabs(x - centre), the IEEE operation np.abs(data - centre)
performs: bit equality.  The mean kinds sum in another order than numpy:
rtol 1e-12 plus, per column, atol = 2 R 2^-53 mean|t| with t the summed
quantity's argument (x for MEAN_AD, BIAS, RMSD; |x - o| for MEAN_AD_TO_OBS and
STD_TO_OBS; CMEAN_AD is the sum of one of each, so it gets the sum of the two
bounds) -- the worst-case bound of fixed-precision summation in any order,
once for numpy's sum and once for the kernel's.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MEDIAN_KINDS = ("mad", "mad_to_obs", "cmad")
MEAN_KINDS = ("mean_ad", "bias", "rmsd", "mean_ad_to_obs", "cmean_ad", "std_to_obs")
KIND_OF = {
    "median_absolute_deviation": "mad",
    "mean_absolute_deviation": "mean_ad",
    "standard_deviation": "std",
    "bias": "bias",
    "root_mean_square_deviation": "rmsd",
    "median_absolute_deviation_to_observation": "mad_to_obs",
    "mean_absolute_deviation_to_observation": "mean_ad_to_obs",
    "combined_median_absolute_deviation": "cmad",
    "combined_mean_absolute_deviation": "cmean_ad",
    "standard_deviation_to_observation": "std_to_obs",
}

# the reference's formulas (scale.py:38-135) for one column x, observation o
FORMULA = {
    "mad": lambda x, o: np.median(np.abs(x - np.median(x))),
    "mean_ad": lambda x, o: np.mean(np.abs(x - np.mean(x))),
    "std": lambda x, o: np.std(x),
    "bias": lambda x, o: np.abs(np.mean(x) - o),
    "rmsd": lambda x, o: np.sqrt(np.abs(np.mean(x) - o) ** 2 + np.std(x) ** 2),
    "mad_to_obs": lambda x, o: np.median(np.abs(x - o)),
    "mean_ad_to_obs": lambda x, o: np.mean(np.abs(x - o)),
    "cmad": lambda x, o: (np.median(np.abs(x - np.median(x)))
                          + np.median(np.abs(x - o))),
    "cmean_ad": lambda x, o: (np.mean(np.abs(x - np.mean(x)))
                              + np.mean(np.abs(x - o))),
    "std_to_obs": lambda x, o: np.std(np.abs(x - o)),
}


@pytest.fixture(scope="module")
def dev():
    from pyabc_amd import gpu
    return gpu.require_device()


@pytest.fixture(scope="module")
def gg():
    return np.load(os.path.join(GOLDEN, "scales.npz"))


def T(a):
    from pyabc_amd import gpu
    return gpu.as_dev(a)


def numpy_scale(kind, X, o):
    """The reference formula per column (each column contiguous, as the
    reference's per-key list is)."""
    Xt = np.ascontiguousarray(X.T)
    return np.array([FORMULA[kind](Xt[j], o[j]) for j in range(X.shape[1])])


def median_scale(kind, X, o):
    """The median kinds over all columns at once (order statistics: the same
    bits as the per-column form)."""
    mad = np.median(np.abs(X - np.median(X, axis=0)), axis=0)
    mado = np.median(np.abs(X - o), axis=0)
    return {"mad": mad, "mad_to_obs": mado, "cmad": mad + mado}[kind]


def mean_atol(kind, X, o):
    R = X.shape[0]
    unit = 2.0 * R * 2.0 ** -53
    ax = np.mean(np.abs(X), axis=0)
    ao = np.mean(np.abs(X - o), axis=0)
    return unit * {"mean_ad": ax, "bias": ax, "rmsd": ax, "std": ax, "mean_ad_to_obs": ao,
                   "std_to_obs": ao, "cmean_ad": ax + ao}[kind]


def check_mean_kind(kind, got, X, o, ref=None, msg=""):
    ref = numpy_scale(kind, X, o) if ref is None else ref
    tol = 1e-12 * np.abs(ref) + mean_atol(kind, X, o)
    err = np.abs(got - ref)
    used = float(np.max(err / np.where(tol > 0, tol, 1.0)))
    print(f"{msg} {kind}: max err / bound = {used:.3g}")
    assert np.all(err <= tol), (msg, kind, err, tol)


def scale_dev(X, kind, o=None):
    from pyabc_amd import gpu
    return gpu.column_scale(T(X), kind, None if o is None else T(o)).cpu().numpy()


# ---- 1. golden ---------------------------------------------------------------

@pytest.mark.parametrize("R", [100, 101])
def test_column_scale_golden(dev, gg, R):
    data, x0 = gg[f"R{R}__data"], gg[f"R{R}__x0"]
    for name, kind in KIND_OF.items():
        got = scale_dev(data, kind, x0)
        ref = gg[f"R{R}_{name}__scales"]
        if kind in MEDIAN_KINDS:
            np.testing.assert_array_equal(got, ref, err_msg=name)
        else:       # "std" (abc_column_std's sums) under the same bound, t = x
            check_mean_kind(kind, got, data, x0, ref=ref, msg=f"golden R={R}")


@pytest.mark.parametrize("R", [100, 101])
@pytest.mark.parametrize("form", ["matrix", "dicts"])
def test_adaptive_weights_golden(dev, gg, R, form):
    import pyabc_amd as pa
    from pyabc_amd.distance import scale
    data, x0v = gg[f"R{R}__data"], gg[f"R{R}__x0"]
    keys = [f"y{k}" for k in range(data.shape[1])]
    x0 = dict(zip(keys, x0v.tolist()))
    for name in KIND_OF:
        for ratio in (None, 5.0):
            if form == "matrix":
                ss = pa.distance.SumStatMatrix(T(data), keys)
            else:
                ss = [dict(zip(keys, row.tolist())) for row in data]
            dist = pa.AdaptivePNormDistance(scale_function=getattr(scale, name),
                                            max_weight_ratio=ratio)
            dist.initialize(0, lambda: ss, x0)
            w = np.array([dist.weights[0][k] for k in keys])
            np.testing.assert_allclose(w, gg[f"R{R}_{name}_r{ratio}__w"], rtol=1e-12,
                                       atol=0, err_msg=f"{name} r{ratio}")
            if form == "matrix":
                assert ss._list is None, name     # never materialised on the host


# ---- 2. median kinds, bit-exact ------------------------------------------------

def edge_matrix(rng, R):
    """The edge matrix of test_gpu_kernels.test_column_mad_select_edges."""
    X = np.empty((R, 9))
    X[:, 0] = 3.25                                  # constant
    X[:, 1] = rng.choice([-0.0, 0.0, 1.0, -1.0], R)  # signed zeros, ties
    X[:, 2] = rng.standard_normal(R)                 # sign mix
    X[:, 3] = np.round(rng.standard_normal(R) * 3)   # heavy ties
    X[:, 4] = rng.standard_normal(R) * 1e-300        # subnormal-ish scale
    X[:, 5] = rng.standard_normal(R) * 1e300
    X[:, 6] = np.exp(rng.standard_normal(R) * 20)    # many exponents
    X[:, 7] = 1.0 + rng.integers(0, 3, R) * 2.0 ** -52  # last-bit ties
    X[:, 8] = -np.abs(rng.standard_normal(R))
    if R >= 8192:
        # sample-bracket misses: huge values at evenly spaced sample rows
        X = np.concatenate([X, rng.standard_normal((R, 1))], 1)
        X[(2 * np.arange(2048) + 1) * R // 4096, 9] = 1e9
    return X


@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 1000, 4096, 65537])
def test_median_kinds_bit_exact(dev, R):
    X = edge_matrix(np.random.default_rng(8 + R), R)
    S = X.shape[1]
    zeros = np.zeros(S)
    zeros[1::2] = -0.0
    obs = {"zeros": zeros, "median": np.median(X, axis=0), "max+1": X.max(axis=0) + 1.0}
    with np.errstate(over="ignore"):
        for oname, o in obs.items():
            for kind in MEDIAN_KINDS:
                np.testing.assert_array_equal(scale_dev(X, kind, o), median_scale(kind, X, o),
                                              err_msg=f"R={R} {kind} o={oname}")


# ---- 3. mean kinds within the a-priori bound -----------------------------------

MEAN_SHAPES = ([(R, 3) for R in (1, 2, 255, 256, 257, 2047, 2048, 2049)]
               + [(4097, S) for S in (1, 10, 255, 256, 257, 600)] + [(20000, 256)])


def mean_case(R, S, seed=5):
    """Columns of scale 10^U(-2, 2); a constant 3.25 with o = 1; 1e6 + N(0, 1)
    with o = 1e6 + 0.5 (|mean| / sigma = 1e6); a rounded column with ties."""
    rng = np.random.default_rng(seed + 1000 * R + S)
    mag = 10.0 ** rng.uniform(-2, 2, S)
    X = rng.standard_normal((R, S)) * mag
    o = rng.standard_normal(S) * mag
    const = big = tied = None
    if S == 3:
        tied, const, big = 0, 1, 2
    elif S >= 2:
        const = 1
        if S >= 4:
            big, tied = 2, 3
    if const is not None:
        X[:, const], o[const] = 3.25, 1.0
    if big is not None:
        X[:, big], o[big] = 1e6 + rng.standard_normal(R), 1e6 + 0.5
    if tied is not None:
        X[:, tied], o[tied] = np.round(rng.standard_normal(R) * 3), 1.0
    return X, o, const


@pytest.mark.parametrize("R,S", MEAN_SHAPES)
def test_mean_kinds_within_bound(dev, R, S):
    X, o, const = mean_case(R, S)
    for kind in MEAN_KINDS:
        got = scale_dev(X, kind, o)
        ref = numpy_scale(kind, X, o)
        check_mean_kind(kind, got, X, o, ref=ref, msg=f"({R}, {S})")
        if const is not None:
            # sums of 3.25 and 2.25 are exact: no rounding anywhere
            assert got[const] == ref[const], (kind, got[const], ref[const])


# ---- 4. unchanged kinds ---------------------------------------------------------

@pytest.mark.parametrize("R,S", [(4097, 3), (20000, 256)])
def test_std_and_mad_unchanged(dev, R, S):
    from pyabc_amd import gpu
    X, o, _ = mean_case(R, S)
    Xd = T(X)
    np.testing.assert_array_equal(gpu.column_scale(Xd, "std").cpu().numpy(),
                                  gpu.column_std(Xd).cpu().numpy())
    np.testing.assert_array_equal(gpu.column_scale(Xd, "mad", T(o)).cpu().numpy(),
                                  gpu.column_mad(Xd).cpu().numpy())


# ---- 5. determinism --------------------------------------------------------------

@pytest.mark.parametrize("R,S", [(20000, 256), (65537, 10)])
def test_bitwise_reproducible(dev, R, S):
    from pyabc_amd import gpu, _native as nat
    X, o, _ = mean_case(R, S)
    Xd, od = T(X), T(o)
    for kind in nat.SCALE_KINDS:
        a = gpu.column_scale(Xd, kind, od).cpu().numpy()
        b = gpu.column_scale(Xd, kind, od).cpu().numpy()
        np.testing.assert_array_equal(a, b, err_msg=kind)


# ---- 6. arguments ----------------------------------------------------------------

def test_bad_arguments_raise(dev):
    from pyabc_amd import gpu, _native as nat
    R, S = 64, 5
    X = T(np.ones((R, S)))
    x0, out = T(np.zeros(S)), T(np.zeros(S))
    ws = gpu.workspace(max(nat.query("abc_column_scale_workspace", k, R, S)
                           for k in range(10)), "colstats")
    st = gpu.stream_ptr()

    def call(kind, R_=R, S_=S, x0p=x0.data_ptr(), nbytes=ws.numel()):
        nat.call("abc_column_scale", kind, X.data_ptr(), R_, S_, x0p, out.data_ptr(),
                 ws.data_ptr(), nbytes, st)

    def last():
        return nat.load().abc_last_error().decode()

    for bad in (-1, 10):
        with pytest.raises(ValueError):
            call(bad)
        assert "column_scale" in last() and "kind" in last()
        assert nat.query("abc_column_scale_workspace", bad, R, S) == 0
    for kind in ("bias", "rmsd", "mad_to_obs", "mean_ad_to_obs", "cmad", "cmean_ad",
                 "std_to_obs"):
        with pytest.raises(ValueError):
            call(nat.SCALE_KINDS[kind], x0p=None)
        assert "column_scale" in last() and "x0" in last()
    for kind in ("mad", "mean_ad", "std"):       # these do not read x0
        call(nat.SCALE_KINDS[kind], x0p=None)
    with pytest.raises(ValueError):
        call(nat.ABC_SCALE_BIAS, R_=0)
    assert "column_scale" in last()
    with pytest.raises(ValueError):
        call(nat.ABC_SCALE_BIAS, S_=0)
    assert "column_scale" in last()
    for kind in range(10):
        need = nat.query("abc_column_scale_workspace", kind, R, S)
        with pytest.raises(nat.NativeError) as ei:
            call(kind, nbytes=need - 1)
        assert ei.value.code == nat.ABC_ERR_WORKSPACE
        assert "column_scale" in last() and "workspace" in last()
    torch.cuda.synchronize()


# ---- 7. end to end -----------------------------------------------------------------

@pytest.mark.parametrize("name", ["root_mean_square_deviation",
                                  "combined_median_absolute_deviation"])
def test_adaptive_run_stays_on_device(dev, name):
    """The test_adaptive_distance_run model with an observation-aware scale
    function: every scale update gets the recorded matrix on the device,
    leaves it there, and equals the numpy formula on that matrix."""
    import pyabc_amd as pa
    from pyabc_amd.distance import SumStatMatrix, scale
    np.random.seed(1)
    rng = np.random.default_rng(1234)
    S = 32
    names = [f"t{k}" for k in range(4)]
    keys = [f"s{k:03d}" for k in range(S)]
    a = rng.uniform(0.5, 2, S)
    sig = 10 ** rng.uniform(-1, 1, S)
    model = pa.LinearGaussianModel(names, keys, src=np.arange(S) % 4, a=a, sigma=sig)
    prior = pa.Distribution(**{n: pa.RV("norm", 0, 1) for n in names})
    x0 = dict(zip(keys, a * 0.5))
    kind = KIND_OF[name]
    dist = pa.AdaptivePNormDistance(scale_function=getattr(scale, name))
    calls = []
    inner = dist._scales

    def recording_scales(all_sum_stats, ks):
        got = np.array(inner(all_sum_stats, ks))
        # the matrix as this call saw it (a device copy: later rounds may
        # reuse the recorded buffer)
        seen = (all_sum_stats.data.clone()
                if isinstance(all_sum_stats, SumStatMatrix) else None)
        calls.append((all_sum_stats, list(ks), got, seen))
        return got

    dist._scales = recording_scales
    abc = pa.ABCSMC(model, prior, dist, population_size=2000,
                    sampler=pa.BatchedGPUSampler(seed=2))
    abc.new("sqlite://", x0)
    h = abc.run(max_nr_populations=3)
    assert h.max_t == 2
    assert len(calls) >= 3
    o = np.array([x0[k] for k in keys])
    for ss, ks, got, seen in calls:
        assert isinstance(ss, SumStatMatrix) and ks == keys and ss.keys == keys
        assert ss._list is None
        X = seen.cpu().numpy()
        assert X.shape[1] == S and X.shape[0] >= 2000
        if kind in MEDIAN_KINDS:
            np.testing.assert_array_equal(got, median_scale(kind, X, o))
        else:
            check_mean_kind(kind, got, X, o, msg=f"run R={X.shape[0]}")
    w_last = dist.weights[max(dist.weights)]
    assert len(w_last) == S and np.isclose(np.mean(list(w_last.values())), 1)
