"""AggregatedDistance / AdaptiveAggregatedDistance on the host: the exports,
the reference's dict helpers and config (pyabc/distance/distance.py:463-507),
when the class offers its device form, pickling, and every argument error of
abc_aggregate_distance, abc_aggregate_accept and abc_column_span -- all
raised before the first device call, so none of this needs a GPU."""
import ctypes as C
import pickle

import numpy as np
import pytest


def children():
    import pyabc_amd as pa
    return [pa.PNormDistance(p=1, weights={"a": 1.0}),
            pa.PNormDistance(p=2, weights={"b": 1.0, "c": 2.0}),
            pa.AdaptivePNormDistance(p=np.inf)]


def test_exports():
    import pyabc_amd as pa
    from pyabc_amd import distance
    from pyabc_amd.distance import aggregate
    assert pa.AggregatedDistance is distance.AggregatedDistance is aggregate.AggregatedDistance
    assert pa.AdaptiveAggregatedDistance is distance.AdaptiveAggregatedDistance
    assert issubclass(pa.AdaptiveAggregatedDistance, pa.AggregatedDistance)
    assert issubclass(pa.AggregatedDistance, pa.Distance)


def test_signatures_and_header_agree():
    """The three entries are declared in include/abcgpu.h with the argument
    counts _native.SIGNATURES binds, and exported by the library."""
    import os
    import re
    from conftest import ROOT
    from pyabc_amd import _native as nat
    src = open(os.path.join(ROOT, "include", "abcgpu.h")).read()
    for name in ("abc_aggregate_distance", "abc_aggregate_accept", "abc_column_span"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", src)
        assert m, name
        assert len(m.group(1).split(",")) == len(nat.SIGNATURES[name][1]), name
        assert hasattr(nat.load(), name)
    assert "#define ABC_AGG_MAX_TERMS 16" in src and nat.ABC_AGG_MAX_TERMS == 16


def test_format_dict_and_latest():
    from pyabc_amd import AggregatedDistance as A
    w = A.format_dict(None, 3, 4)
    assert list(w) == [3] and np.array_equal(w[3], np.ones(4))
    w = A.format_dict(None, 0, 2, default_val=0.5)
    assert np.array_equal(w[0], [0.5, 0.5])
    w = A.format_dict([1, 2, 3], 5, 3)
    assert list(w) == [5] and isinstance(w[5], np.ndarray) and np.array_equal(w[5], [1, 2, 3])
    by_t = {0: [1.0, 2.0], 4: [3.0, 4.0]}
    assert A.format_dict(by_t, 7, 2) is by_t        # a dict is by t already
    assert A.get_for_t_or_latest(by_t, 0) == [1.0, 2.0]
    assert A.get_for_t_or_latest(by_t, 2) == [3.0, 4.0]     # absent: the latest
    assert A.get_for_t_or_latest(by_t, 9) == [3.0, 4.0]


def test_term_weights_list_and_dict():
    import pyabc_amd as pa
    d = pa.AggregatedDistance(children(), weights=[1.0, 0.5, 2.0], factors=[2.0, 1.0, 0.25])
    np.testing.assert_array_equal(d.term_weights(0), [2.0, 0.5, 0.5])
    d = pa.AggregatedDistance(children(), weights={0: [1.0, 0.5, 2.0], 2: [0.3, 1.7, 0.9]},
                              factors={0: [1.5, 1.0, 0.5]})
    np.testing.assert_array_equal(d.term_weights(0), np.array([1.0, 0.5, 2.0]) * [1.5, 1.0, 0.5])
    np.testing.assert_array_equal(d.term_weights(5), np.array([0.3, 1.7, 0.9]) * [1.5, 1.0, 0.5])
    # a single distance is wrapped in a list, a callable in a distance
    one = pa.AggregatedDistance(lambda x, y: 1.0)
    assert len(one.distances) == 1 and isinstance(one.distances[0], pa.SimpleFunctionDistance)


def test_get_config():
    import pyabc_amd as pa
    ch = children()
    conf = pa.AggregatedDistance(ch).get_config()
    assert list(conf) == ["Distance_0", "Distance_1", "Distance_2"]
    for j in range(3):
        assert conf[f"Distance_{j}"] == ch[j].get_config()
    assert conf["Distance_2"]["name"] == "AdaptivePNormDistance"
    ada = pa.AdaptiveAggregatedDistance(children())
    assert list(ada.get_config()) == list(conf)


def test_adaptive_constructor_follows_reference():
    import pyabc_amd as pa
    from pyabc_amd.distance import scale
    ada = pa.AdaptiveAggregatedDistance(children())
    assert ada.scale_function is scale.span and ada.adaptive and ada.log_file is None
    assert ada.initial_weights is None and ada.weights is None and ada.x_0 is None

    class FakeSampler:
        class sample_factory:
            record_rejected = False
    # only the children turn record_rejected on: two plain p-norms leave it off
    pa.AdaptiveAggregatedDistance(children()[:2]).configure_sampler(FakeSampler)
    assert FakeSampler.sample_factory.record_rejected is False
    ada.configure_sampler(FakeSampler)          # the AdaptivePNormDistance child
    assert FakeSampler.sample_factory.record_rejected is True


def test_initial_weights_and_log_file(tmp_path):
    import pyabc_amd as pa
    from pyabc_amd.storage.json import load_dict_from_json
    x0 = {"a": 0.0, "b": 1.0, "c": 2.0}
    log = tmp_path / "w.json"
    ch = [pa.PNormDistance(p=1), pa.PNormDistance(p=2)]
    ada = pa.AdaptiveAggregatedDistance(ch, initial_weights=[3.0, 4.0], adaptive=False,
                                        log_file=str(log))

    def no_stats():
        raise AssertionError("initial_weights: no sum stats are requested")
    ada.initialize(0, no_stats, x0)
    assert ada.weights[0] == [3.0, 4.0] and ada.x_0 is x0
    np.testing.assert_array_equal(ada.term_weights(0), [3.0, 4.0])
    assert ada.update(1, no_stats) is False     # adaptive=False: pre-calibration only
    ada.weights[1] = np.array([0.5, 0.25])
    ada.log(1)
    assert load_dict_from_json(str(log)) == {0: [3.0, 4.0], 1: [0.5, 0.25]}


def test_batched_capable_cases():
    import pyabc_amd as pa
    assert pa.AggregatedDistance(children()).batched_capable
    assert pa.AdaptiveAggregatedDistance(children()).batched_why_not == ""

    fn = pa.AggregatedDistance([pa.PNormDistance(p=1), lambda x, y: 0.0])
    assert not fn.batched_capable
    assert "child 1" in fn.batched_why_not and "SimpleFunctionDistance" in fn.batched_why_not

    class Shifted(pa.PNormDistance):
        def __call__(self, x, x_0, t=None, par=None):
            return 1.0 + super().__call__(x, x_0, t, par)
    sub = pa.AggregatedDistance([Shifted(p=2), pa.PNormDistance(p=1)])
    assert not sub.batched_capable
    assert "child 0" in sub.batched_why_not and "Shifted" in sub.batched_why_not
    with pytest.raises(TypeError, match="Shifted"):
        sub.term_stack(0, ["a"], "cpu")

    k16 = pa.AggregatedDistance([pa.PNormDistance(p=1) for _ in range(16)])
    assert k16.batched_capable
    k17 = pa.AggregatedDistance([pa.PNormDistance(p=1) for _ in range(17)])
    assert not k17.batched_capable and "17" in k17.batched_why_not

    # the per-candidate form calls children through their own __call__
    agg = pa.AggregatedDistance([lambda x, y: 2.0, lambda x, y: x["a"] - y["a"]],
                                weights=[1.0, 10.0])
    assert agg({"a": 3.0}, {"a": 1.0}, 0) == 22.0


def test_pickle_round_trip():
    import pyabc_amd as pa
    ada = pa.AdaptiveAggregatedDistance(children(), initial_weights=[1.0, 2.0, 3.0],
                                        factors=[1.0, 0.5, 0.25])
    ada._dev_stack_cache["sentinel"] = object()      # stands for device tensors
    back = pickle.loads(pickle.dumps(ada))
    assert back._dev_stack_cache == {}
    assert "sentinel" in ada._dev_stack_cache        # the original keeps its cache
    assert back.initial_weights == [1.0, 2.0, 3.0] and back.factors == [1.0, 0.5, 0.25]
    assert back.scale_function is ada.scale_function
    assert [type(d) for d in back.distances] == [type(d) for d in ada.distances]
    assert [d.p for d in back.distances] == [1, 2, np.inf]
    assert back.batched_capable


# ---- argument errors: raised before any device call ---------------------------

def arr(*v):
    return (C.c_double * len(v))(*v)


@pytest.fixture()
def natlib():
    from pyabc_amd import _native as nat
    nat.load()
    return nat


def last(nat):
    return nat.load().abc_last_error().decode()


X = 0x1000      # stands for a device pointer: never dereferenced by the checks


def agg_distance(nat, x=X, B=4, S=3, x0=X, wf=X, p=None, c=None, K=2, d=X, terms=X):
    p = arr(1.0, 2.0) if p is None else p
    c = arr(1.0, 1.0) if c is None else c
    nat.call("abc_aggregate_distance", x, B, S, x0, wf, p, c, K, d, terms, None)


def agg_accept(nat, ws, nbytes, x=X, B=4, S=3, x0=X, wf=X, p=None, c=None, K=2, cap=4,
               idx=X, count=X):
    p = arr(1.0, 2.0) if p is None else p
    c = arr(1.0, 1.0) if c is None else c
    nat.call("abc_aggregate_accept", x, B, S, x0, wf, p, c, K, 1.0, None, 0, cap, idx,
             count, ws, nbytes, None)


BAD_TERMS = [
    (dict(K=0), "K outside"),
    (dict(K=17, p=arr(*[1.0] * 17), c=arr(*[1.0] * 17)), "K outside"),
    (dict(p=arr(1.0, 0.5)), "p < 1"),
    (dict(p=arr(float("nan"), 1.0)), "p < 1"),
    (dict(p=C.cast(None, C.c_void_p)), "null pointer"),
    (dict(c=C.cast(None, C.c_void_p)), "null pointer"),
    (dict(B=-1), "B"),
    (dict(S=0), "S < 1"),
    (dict(x=None), "null pointer"),
    (dict(x0=None), "null pointer"),
    (dict(wf=None), "null pointer"),
]


@pytest.mark.parametrize("kw,word", BAD_TERMS)
def test_aggregate_distance_argument_errors(natlib, kw, word):
    with pytest.raises(ValueError):
        agg_distance(natlib, **kw)
    assert "aggregate_distance" in last(natlib) and word in last(natlib)


def test_aggregate_distance_needs_an_output(natlib):
    with pytest.raises(ValueError):
        agg_distance(natlib, d=None, terms=None)
    assert "aggregate_distance" in last(natlib) and "both outputs null" in last(natlib)
    agg_distance(natlib, B=0, x=None, d=None)      # B = 0: nothing to do, no error


@pytest.mark.parametrize("kw,word", BAD_TERMS + [(dict(count=None), "null pointer"),
                                                 (dict(idx=None), "null pointer"),
                                                 (dict(cap=-1), "cap")])
def test_aggregate_accept_argument_errors(natlib, kw, word):
    ws = C.create_string_buffer(1 << 16)
    with pytest.raises(ValueError):
        agg_accept(natlib, C.addressof(ws), len(ws), **kw)
    assert "aggregate_accept" in last(natlib) and word in last(natlib)


def test_aggregate_accept_short_workspace(natlib):
    need = natlib.query("abc_candidates_workspace", 4)
    ws = C.create_string_buffer(need)
    with pytest.raises(natlib.NativeError) as ei:
        agg_accept(natlib, C.addressof(ws), need - 1)
    assert ei.value.code == natlib.ABC_ERR_WORKSPACE
    assert "aggregate_accept" in last(natlib) and "workspace" in last(natlib)


def test_column_span_argument_errors(natlib):
    need = natlib.query("abc_column_stats_workspace", 10, 3)
    ws = C.create_string_buffer(need)

    def span(V=X, R=10, K=3, out=X, nbytes=need):
        natlib.call("abc_column_span", V, R, K, out, C.addressof(ws), nbytes, None)

    for kw, word in ((dict(R=0), "bad R"), (dict(R=(1 << 31) + 1), "bad R"),
                     (dict(K=0), "K outside"), (dict(K=257), "K outside"),
                     (dict(V=None), "null pointer"), (dict(out=None), "null pointer")):
        with pytest.raises(ValueError):
            span(**kw)
        assert "column_span" in last(natlib) and word in last(natlib), kw
    with pytest.raises(natlib.NativeError) as ei:
        span(nbytes=need - 1)
    assert ei.value.code == natlib.ABC_ERR_WORKSPACE
    assert "column_span" in last(natlib) and "workspace" in last(natlib)
