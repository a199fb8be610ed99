"""The measure-list distances on the host (no GPU): the reference's interface
and arithmetic (pyabc/distance/distance.py:634-873) against
tests/golden/measure_list.npz, and the vectors their device forms are made
from."""
import pickle

import numpy as np
import pytest

import measure_list_ref as ref

CLASSES = ("zscore", "pca", "minmax", "percentile")


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture()


def make(name, measures="all"):
    import pyabc_amd as pa
    cls = {"zscore": pa.ZScoreDistance, "pca": pa.PCADistance,
           "minmax": pa.MinMaxDistance, "percentile": pa.PercentileDistance}[name]
    return cls(measures_to_use=measures)


def initialized(fx, name, tag, measures="all"):
    sample = ref.sample_of(fx, tag[0])
    stats = ref.as_dicts(sample)
    x0 = dict(zip(ref.keys(sample.shape[1]), fx[f"{tag[0]}__x0"]))
    dist = make(name, measures)
    dist.initialize(0, lambda: stats, x0)
    return dist, x0


def close(got, want, rel):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= rel * np.abs(want)), np.max(
        np.abs(got - want) / np.abs(want))


def test_exports_and_constructors():
    import pyabc_amd as pa
    import pyabc_amd.distance as pd
    names = ("DistanceWithMeasureList", "ZScoreDistance", "PCADistance",
             "RangeEstimatorDistance", "MinMaxDistance", "PercentileDistance")
    for n in names:
        assert getattr(pa, n) is getattr(pd, n)
        assert issubclass(getattr(pa, n), pa.Distance)
    assert issubclass(pa.MinMaxDistance, pa.RangeEstimatorDistance)
    assert issubclass(pa.PercentileDistance, pa.RangeEstimatorDistance)
    for n in names[1:]:
        assert issubclass(getattr(pa, n), pa.DistanceWithMeasureList)
        d = getattr(pa, n)()
        assert d.measures_to_use == "all"
        assert getattr(pa, n)(["b", "a"]).measures_to_use == ["b", "a"]
    assert pa.PercentileDistance.PERCENTILE == 20
    assert pa.PCADistance()._whitening_transformation_matrix is None
    assert pa.MinMaxDistance().normalization is None


def test_get_config(fx):
    ks = ref.keys(10)
    d, _ = initialized(fx, "zscore", "A")
    assert d.get_config() == {"name": "ZScoreDistance", "measures_to_use": ks}
    d, _ = initialized(fx, "pca", "A")
    assert d.get_config() == {"name": "PCADistance", "measures_to_use": ks}
    d, _ = initialized(fx, "minmax", "A")
    c = d.get_config()
    assert set(c) == {"name", "measures_to_use", "normalization"}
    assert c["normalization"] is d.normalization and list(c["normalization"]) == ks
    d, _ = initialized(fx, "percentile", "A")
    assert d.get_config()["PERCENTILE"] == 20
    assert make("minmax", ["y1"]).get_config()["measures_to_use"] == ["y1"]


@pytest.mark.parametrize("tag", ("A", "B", "C", "A_sub"))
@pytest.mark.parametrize("name", CLASSES)
def test_initialize_and_call_reproduce_the_reference(fx, name, tag):
    measures = [f"y{k}" for k in fx["SUBSET"]] if tag == "A_sub" else "all"
    dist, x0 = initialized(fx, name, tag, measures)
    S = len(x0)
    use = list(fx["SUBSET"]) if tag == "A_sub" else list(range(S))
    assert dist.measures_to_use == [f"y{k}" for k in use]
    if name in ("minmax", "percentile"):
        got = np.array([dist.normalization[k] for k in dist.measures_to_use])
        # the same host arithmetic on the same values
        np.testing.assert_array_equal(got, fx[f"{tag}_{name}__norm"])
    if name == "pca":
        W = fx[f"{tag}_pca__W"]
        got = dist._whitening_transformation_matrix
        # the reference's own numpy and scipy calls on the same values
        assert np.max(np.abs(got - W)) <= 1e-12 * np.max(np.abs(W))
    rows = ref.as_dicts(fx[f"{tag[0]}__rows"])
    d = np.array([dist(r, x0) for r in rows])
    close(d, fx[f"{tag}_{name}__d"], 1e-12)


@pytest.mark.parametrize("tag", ("A", "A_sub"))
def test_weight_vectors(fx, tag):
    measures = [f"y{k}" for k in fx["SUBSET"]] if tag == "A_sub" else "all"
    use = list(fx["SUBSET"]) if tag == "A_sub" else list(range(10))
    ks = ref.keys(10)
    for name in ("minmax", "percentile"):
        dist, x0 = initialized(fx, name, tag, measures)
        want = np.zeros(10)
        want[use] = 1.0 / fx[f"{tag}_{name}__norm"]
        np.testing.assert_array_equal(dist.weight_vector(0, ks), want)
    dist, x0 = initialized(fx, "zscore", tag, measures)
    want = np.zeros(10)
    want[use] = 1.0 / (np.abs(fx["A__x0"][use]) * len(use))
    np.testing.assert_array_equal(dist.weight_vector(0, ks), want)
    # the weighted 1-norm is the reference's distance
    X, o = fx["A__rows"], fx["A__x0"]
    d = np.abs(dist.weight_vector(0, ks) * (X - o)).sum(axis=1)
    close(d, fx[f"{tag}_zscore__d"], 1e-12)
    dist, x0 = initialized(fx, "pca", tag, measures)
    W = dist.whitening_matrix(ks)
    assert W.shape == (10, 10)
    np.testing.assert_array_equal(W[np.ix_(use, use)], dist._whitening_transformation_matrix)
    rest = [k for k in range(10) if k not in use]
    assert not W[rest].any() and not W[:, rest].any()
    d, _ = ref.whitened(X, o, W)
    close(d, [dist(r, x0) for r in ref.as_dicts(X)], 1e-12)


def test_zero_normalization_is_an_infinite_weight():
    import pyabc_amd as pa
    stats = [{"a": 1.0, "b": 2.0}, {"a": 1.0, "b": 3.0}]
    d = pa.MinMaxDistance()
    d.initialize(0, lambda: stats, {"a": 1.0, "b": 2.5})
    np.testing.assert_array_equal(d.weight_vector(0, ["a", "b"]), [np.inf, 1.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        assert d({"a": np.float64(2.0), "b": np.float64(2.5)}, {"a": 1.0, "b": 2.5}) == np.inf
        assert np.isnan(d({"a": np.float64(1.0), "b": np.float64(2.5)}, {"a": 1.0, "b": 2.5}))


def test_zscore_zero_observation(fx):
    import pyabc_amd as pa
    ks = ref.keys(3)
    x0 = dict(zip(ks, fx["Z__x0"]))
    z = pa.ZScoreDistance()
    assert z.batched_capable           # nothing known before initialize
    z.initialize(0, lambda: ref.as_dicts(ref.sample_of(fx, "C")), x0)
    assert z.batched_capable is False
    assert z.batched_why_not == "ZScoreDistance with a zero observation"
    d = np.array([z(r, x0) for r in ref.as_dicts(fx["Z__rows"])])
    want = fx["Z_zscore__d"]
    assert np.all(np.isinf(want[50:])) and np.all(np.isfinite(want[:50]))
    np.testing.assert_array_equal(np.isinf(d), np.isinf(want))
    close(d[:50], want[:50], 1e-12)
    # a zero observation outside the measures does not matter
    z2 = pa.ZScoreDistance(["y2", "y0"])
    z2.initialize(0, lambda: [], x0)
    assert z2.batched_capable and z2.batched_why_not == ""
    np.testing.assert_array_equal(
        z2.weight_vector(0, ks), [1 / (abs(x0["y0"]) * 2), 0.0, 1 / (abs(x0["y2"]) * 2)])


def test_percentile_is_read_at_initialize(fx, monkeypatch):
    import pyabc_amd as pa
    monkeypatch.setattr(pa.PercentileDistance, "PERCENTILE", 10)
    dist, _ = initialized(fx, "percentile", "C")
    sample = ref.sample_of(fx, "C")
    want = np.percentile(sample, 90, axis=0) - np.percentile(sample, 10, axis=0)
    close([dist.normalization[k] for k in ref.keys(3)], want, 1e-15)
    assert dist.get_config()["PERCENTILE"] == 10


def test_user_subclasses(fx):
    import pyabc_amd as pa

    class Quartiles(pa.RangeEstimatorDistance):
        @staticmethod
        def lower(parameter_list):
            return np.percentile(parameter_list, 25)

        @staticmethod
        def upper(parameter_list):
            return np.percentile(parameter_list, 75)

    sample = ref.sample_of(fx, "C")
    x0 = dict(zip(ref.keys(3), fx["C__x0"]))
    d = Quartiles()
    d.initialize(0, lambda: ref.as_dicts(sample), x0)
    iqr = np.percentile(sample, 75, axis=0) - np.percentile(sample, 25, axis=0)
    close([d.normalization[k] for k in ref.keys(3)], iqr, 1e-15)
    rows = fx["C__rows"]
    close([d(r, x0) for r in ref.as_dicts(rows)],
          ref.ranged(rows, fx["C__x0"], iqr, range(3)), 1e-12)
    # still a weighted 1-norm: the batched forms apply
    assert d.batched_capable and hasattr(d, "fused_pnorm")
    np.testing.assert_array_equal(d.weight_vector(0, ref.keys(3)), 1.0 / iqr)

    class Halved(pa.MinMaxDistance):
        def __call__(self, x, x_0, t=None, par=None):
            return 0.5 * super().__call__(x, x_0, t, par)

    h = Halved()
    assert not h.batched_capable and "Halved" in h.batched_why_not
    assert h.fused_pnorm(0, ref.keys(3), None) is None

    class Own(pa.DistanceWithMeasureList):
        def __call__(self, x, x_0, t=None, par=None):
            return sum(abs(x[k] - x_0[k]) for k in self.measures_to_use)

    o = Own()
    o.initialize(0, lambda: [], x0)
    assert o.measures_to_use == ref.keys(3)
    assert not hasattr(o, "device_call")     # the sampler's per-candidate loop


def test_pca_over_too_many_statistics_names_the_limit():
    import pyabc_amd as pa
    rng = np.random.default_rng(0)
    ks = ref.keys(257)
    stats = [dict(zip(ks, rng.normal(size=257))) for _ in range(300)]
    d = pa.PCADistance()
    d.initialize(0, lambda: stats, dict(zip(ks, np.zeros(257))))
    assert not d.batched_capable and "256" in d.batched_why_not


def test_pickle_drops_device_state(fx):
    dist, _ = initialized(fx, "pca", "C")
    dist.__dict__["_dev_cache"] = {"k": object()}
    back = pickle.loads(pickle.dumps(dist))
    assert back._dev_cache == {}
    np.testing.assert_array_equal(back._whitening_transformation_matrix,
                                  dist._whitening_transformation_matrix)
