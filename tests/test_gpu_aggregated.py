"""AggregatedDistance / AdaptiveAggregatedDistance on the device:
abc_aggregate_distance, abc_aggregate_accept and abc_column_span against the
entries they are defined by (abc_pnorm per term, abc_accept_compact on the
distance array, numpy's exact max - min), the reference's values in
tests/golden/aggregated.npz, and one adaptive run that stays on the device.

Tolerances.  Terms, the combine, the accept positions and the span are
defined bit for bit: equality.  The goldens carry the reference's own
summation order (np.dot, np.std, Python's sum): 1e-12 relative, the bar of the
p-norm and scale goldens; the generator asserts the margins that keep the
reference's rounding three orders below it.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

P_ALL = (1.0, 2.0, 3.0, 1.5, np.inf)
P_SIMPLE = (1.0, 2.0, np.inf)
S_ALL = (1, 5, 32, 33, 64, 65, 256, 600)
B_ALL = (1, 7, 255, 257, 2047, 2049, 4099)
K_ALL = (1, 2, 3, 16)


@pytest.fixture(scope="module")
def dev():
    from pyabc_amd import gpu
    return gpu.require_device()


def same_bits(got, want, msg=""):
    """Equal as bit patterns, any NaN equal to any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, msg
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=msg)
    np.testing.assert_array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64),
                                  err_msg=msg)


def make_case(rng, B, S, K, pset):
    """x [B, S] with a NaN entry (row 3) and an inf entry (row 5), x0 [S],
    wf [K, S] with a zero-weight key per term, p [K] cycling through pset from
    a random start, c [K]."""
    x = rng.normal(size=(B, S)) * 10.0 ** rng.uniform(-1, 1, size=S)
    if B > 3:
        x[3, rng.integers(S)] = np.nan
    if B > 5:
        x[5, rng.integers(S)] = np.inf
    x0 = rng.normal(size=S)
    wf = rng.uniform(0.1, 2.0, size=(K, S))
    if S > 1:
        wf[np.arange(K), rng.integers(S, size=K)] = 0.0
    start = rng.integers(len(pset))
    p = np.array([pset[(start + k) % len(pset)] for k in range(K)])
    c = rng.uniform(0.2, 3.0, size=K)
    return x, x0, wf, p, c


def combine(terms, c):
    """((0 + c_0 t_0) + c_1 t_1) + ... in k order, one rounding per operation."""
    d = np.zeros(terms.shape[0])
    with np.errstate(invalid="ignore"):
        for k in range(terms.shape[1]):
            d = d + c[k] * terms[:, k]
    return d


# ---- 1. terms and d, bit for bit ------------------------------------------------

@pytest.mark.parametrize("S", S_ALL)
def test_terms_equal_pnorm_and_d_the_ordered_combine(dev, S):
    from pyabc_amd import gpu
    rng = np.random.default_rng(100 + S)
    for B in B_ALL:
        for K in K_ALL:
            for pset in (P_SIMPLE, P_ALL):
                x, x0, wf, p, c = make_case(rng, B, S, K, pset)
                xd, x0d, wfd = gpu.as_dev(x), gpu.as_dev(x0), gpu.as_dev(wf)
                stack = gpu.TermStack(wfd, p, c)
                d, terms = gpu.aggregate_distance(xd, x0d, stack, terms=True)
                want = np.stack([gpu.pnorm(xd, x0d, wfd[k].contiguous(), float(p[k]))
                                 .cpu().numpy() for k in range(K)], axis=1)
                msg = f"S={S} B={B} K={K} p={p}"
                same_bits(terms.cpu().numpy(), want, msg)
                same_bits(d.cpu().numpy(), combine(want, c), msg)
                # each output alone: the same bits
                same_bits(gpu.aggregate_distance(xd, x0d, stack).cpu().numpy(),
                          d.cpu().numpy(), msg)


def test_zero_weight_on_an_infinite_term_is_nan(dev):
    from pyabc_amd import gpu
    x = np.zeros((2, 40))
    x[1, 7] = np.inf
    wf = np.ones((2, 40))
    stack = gpu.TermStack(gpu.as_dev(wf), [1.0, 2.0], [0.0, 1.0])
    d = gpu.aggregate_distance(gpu.as_dev(x), gpu.as_dev(np.zeros(40)), stack).cpu().numpy()
    assert d[0] == 0.0 and np.isnan(d[1])       # 0 * inf, as np.dot


# ---- 2. accept tail ----------------------------------------------------------------

def reference_accept(gpu, xd, x0d, stack, eps, att, max_attempts):
    d = gpu.aggregate_distance(xd, x0d, stack).clone()
    if att is not None:
        gpu.mask_gave_up(d, att, max_attempts)
    idx, cnt = gpu.accept_compact(d, eps)
    n = int(cnt.item())
    return idx[:n].cpu().numpy(), n


@pytest.mark.parametrize("S,B,K,pset", [(5, 4099, 3, P_ALL), (32, 2049, 16, P_SIMPLE),
                                        (33, 2047, 2, P_SIMPLE), (65, 4099, 3, P_ALL),
                                        (256, 257, 16, P_ALL), (600, 7, 3, P_SIMPLE)])
def test_accept_tail_equals_compact_of_the_distances(dev, S, B, K, pset):
    from pyabc_amd import _native as nat
    from pyabc_amd import gpu
    rng = np.random.default_rng(7 * S + B)
    x, x0, wf, p, c = make_case(rng, B, S, K, pset)
    xd, x0d = gpu.as_dev(x), gpu.as_dev(x0)
    stack = gpu.TermStack(gpu.as_dev(wf), p, c)
    d = gpu.aggregate_distance(xd, x0d, stack).cpu().numpy()
    finite = d[np.isfinite(d)]
    att = gpu.as_dev(rng.integers(1, 8, size=B), dtype=torch.int32)
    tie = float(np.sort(finite)[len(finite) // 3])         # one row's exact d
    for eps, a, ma in ((tie, None, 0), (np.inf, None, 0), (float(np.median(finite)), att, 5),
                       (-1.0, None, 0)):
        want_idx, want_n = reference_accept(gpu, xd, x0d, stack, eps, a, ma)
        if eps == tie:
            assert tie in d[want_idx]                      # the tie is accepted
        if eps == np.inf and B > 3:
            assert 3 not in want_idx and want_n < B        # the NaN row never is
        for cap in sorted({0, 1, max(want_n // 2, 1), want_n, B}):
            for _ in range(2):                             # twice on the same workspace
                idx, cnt = gpu.aggregate_accept(xd, x0d, stack, eps, cap, att=a,
                                                max_attempts=ma)
                assert int(cnt.item()) == want_n, (eps, cap)
                m = min(cap, want_n)
                np.testing.assert_array_equal(idx[:m].cpu().numpy(), want_idx[:m])
            ws = gpu.workspace(nat.query("abc_candidates_workspace", B), "candidates")
            assert not ws[:256].any().item()               # the ticket block stays zero


def test_accept_tail_empty_round(dev):
    from pyabc_amd import gpu
    stack = gpu.TermStack(gpu.as_dev(np.ones((2, 40))), [1.0, np.inf], [1.0, 1.0])
    x = torch.empty((0, 40), dtype=torch.float64, device=dev)
    idx, cnt = gpu.aggregate_accept(x, gpu.as_dev(np.zeros(40)), stack, 1.0, 10)
    assert int(cnt.item()) == 0
    assert gpu.aggregate_distance(x, gpu.as_dev(np.zeros(40)), stack).numel() == 0


# ---- 3. abc_column_span ----------------------------------------------------------

@pytest.mark.parametrize("R", [1, 2, 255, 256, 257, 4097, 65537])
@pytest.mark.parametrize("K", [1, 3, 16])
def test_column_span_is_exact(dev, R, K):
    from pyabc_amd import gpu
    rng = np.random.default_rng(R * 31 + K)
    for off in range(5):
        V = rng.normal(size=(R, K)) * 10.0 ** rng.uniform(-3, 3, size=K)
        for k in range(K):
            kind = (k + off) % 5                 # 0: signed values as drawn
            if kind == 1:
                V[:, k] = -3.25                  # constant: exactly 0
            elif kind == 2:
                V[rng.integers(R), k] = np.inf
                V[rng.integers(R), k] = -np.inf  # (may overwrite: then inf - finite)
            elif kind == 3:
                V[rng.integers(R), k] = np.nan
            elif kind == 4:
                V[rng.integers(R), k] = np.inf
        with np.errstate(invalid="ignore"):
            want = V.max(axis=0) - V.min(axis=0)
        got = gpu.column_span(gpu.as_dev(V)).cpu().numpy()
        same_bits(got, want, f"R={R} K={K} off={off}")
        for k in range(K):
            if (k + off) % 5 == 1:
                assert got[k] == 0.0
            if (k + off) % 5 == 3:
                assert np.isnan(got[k])


# ---- 4. goldens --------------------------------------------------------------------

S_G = 12
KEYS = [f"y{k}" for k in range(S_G)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "aggregated.npz"))


def children():
    import pyabc_amd as pa
    return [pa.PNormDistance(p=1, weights={k: 1.0 for k in KEYS[:4]}),
            pa.PNormDistance(p=2, weights={k: 1.0 for k in KEYS[4:]}),
            pa.AdaptivePNormDistance(p=np.inf)]


def stats_in(form, data):
    """The recorded sum stats as the device matrix or as the reference's list."""
    from pyabc_amd import gpu
    from pyabc_amd.distance import SumStatMatrix
    if form == "matrix":
        return SumStatMatrix(gpu.as_dev(data), KEYS)
    return [{k: float(v) for k, v in zip(KEYS, row)} for row in data]


@pytest.mark.parametrize("form", ["matrix", "dicts"])
@pytest.mark.parametrize("R", [100, 101])
def test_golden_distances(dev, gold, R, form):
    import pyabc_amd as pa
    from pyabc_amd import gpu
    data, x0v = gold[f"R{R}__data"], gold[f"R{R}__x0"]
    x0 = dict(zip(KEYS, x0v.tolist()))
    xd, x0d = gpu.as_dev(data), gpu.as_dev(x0v)
    ss = stats_in(form, data)

    agg = pa.AggregatedDistance(children(), weights=gold["LIST_W"].tolist(),
                                factors=gold["LIST_F"].tolist())
    agg.initialize(0, lambda: ss, x0)
    w2 = agg.distances[2].weights[0]
    np.testing.assert_allclose([w2[k] for k in KEYS], gold[f"R{R}__child2_w"], rtol=1e-12)
    _, terms = gpu.aggregate_distance(xd, x0d, agg.term_stack(0, KEYS, dev), terms=True)
    np.testing.assert_allclose(terms.cpu().numpy(), gold[f"R{R}__terms"], rtol=1e-12)
    d = agg.device_call(xd, x0d, 0, KEYS).cpu().numpy()
    np.testing.assert_allclose(d, gold[f"R{R}_list__d"], rtol=1e-12)
    # the per-candidate form, through the children's own __call__
    rows = ss if form == "dicts" else stats_in("dicts", data)
    for i in (0, 17, R - 1):
        np.testing.assert_allclose(agg(rows[i], x0, 0), gold[f"R{R}_list__d"][i], rtol=1e-12)

    agg = pa.AggregatedDistance(
        children(), weights={0: gold["DICT_W_t0"], 2: gold["DICT_W_t2"]},
        factors={0: gold["DICT_F_t0"]})
    agg.initialize(0, lambda: ss, x0)
    for t in (0, 2, 5):                  # 5: falls back to the latest entry
        d = agg.device_call(xd, x0d, t, KEYS).cpu().numpy()
        np.testing.assert_allclose(d, gold[f"R{R}_dict_t{t}__d"], rtol=1e-12)
        np.testing.assert_allclose(agg(rows[3], x0, t), gold[f"R{R}_dict_t{t}__d"][3],
                                   rtol=1e-12)


@pytest.mark.parametrize("form", ["matrix", "dicts"])
@pytest.mark.parametrize("name", ["span", "mean", "median"])
@pytest.mark.parametrize("R", [100, 101])
def test_golden_adaptive_weights(dev, gold, R, name, form):
    import pyabc_amd as pa
    from pyabc_amd.distance import scale
    data, data2, x0v = gold[f"R{R}__data"], gold[f"R{R}__data2"], gold[f"R{R}__x0"]
    x0 = dict(zip(KEYS, x0v.tolist()))
    ss, ss2 = stats_in(form, data), stats_in(form, data2)
    ada = pa.AdaptiveAggregatedDistance(children(), scale_function=getattr(scale, name))
    ada.initialize(0, lambda: ss, x0)
    assert isinstance(ada.weights[0], np.ndarray)
    np.testing.assert_allclose(ada.weights[0], gold[f"R{R}_{name}__w0"], rtol=1e-12)
    assert ada.update(1, lambda: ss2) is True
    w2 = ada.distances[2].weights[1]
    np.testing.assert_allclose([w2[k] for k in KEYS], gold[f"R{R}_{name}__child2_w1"],
                               rtol=1e-12)
    np.testing.assert_allclose(ada.weights[1], gold[f"R{R}_{name}__w1"], rtol=1e-12)
    if form == "matrix":
        assert ss._list is None and ss2._list is None     # never left the device


def test_adaptive_other_callable_gets_lists(dev, gold):
    import pyabc_amd as pa
    data, x0v = gold["R100__data"], gold["R100__x0"]
    x0 = dict(zip(KEYS, x0v.tolist()))
    seen = []

    def spread(values):
        assert isinstance(values, list) and isinstance(values[0], float)
        seen.append(len(values))
        return np.percentile(values, 90) - np.percentile(values, 10)
    ada = pa.AdaptiveAggregatedDistance(children(), scale_function=spread)
    ada.initialize(0, lambda: stats_in("matrix", data), x0)
    assert seen == [100, 100, 100]
    # (interpolated order statistics of terms that agree to ~S 2^-53: the
    # decile spread is of the terms' own size, no cancellation)
    t = gold["R100__terms"]
    want =1 / (np.percentile(t, 90, axis=0) - np.percentile(t, 10, axis=0))
    np.testing.assert_allclose(ada.weights[0], want, rtol=1e-12)


# ---- 5. end to end ------------------------------------------------------------------

def run_adaptive(accept_tail):
    """The test_adaptive_run_stays_on_device model with an
    AdaptiveAggregatedDistance of the three children; returns what each
    generation stored and what each update saw."""
    import pyabc_amd as pa
    from pyabc_amd.distance import SumStatMatrix
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
    dist = pa.AdaptiveAggregatedDistance([
        pa.PNormDistance(p=1, weights={k: 1.0 for k in keys[:4]}),
        pa.PNormDistance(p=2, weights={k: 1.0 for k in keys[4:]}),
        pa.AdaptivePNormDistance(p=np.inf)])
    updates, stored, stats = [], [], []
    inner = dist._term_scales

    def recording_scales(sum_stats):
        got = inner(sum_stats)
        mat = isinstance(sum_stats, SumStatMatrix)
        child = dist.distances[2]
        w2 = child.weights[max(child.weights)]
        updates.append(dict(ss=sum_stats, keys=sum_stats.keys if mat else None,
                            seen=sum_stats.data.clone() if mat else None,
                            child_w=np.array([w2[k] for k in keys]), scales=np.array(got)))
        return got
    dist._term_scales = recording_scales
    sampler = pa.BatchedGPUSampler(seed=2, allow_per_candidate=False,
                                   accept_tail=accept_tail)
    sample_inner = sampler.sample_until_n_accepted

    def recording_sample(*args, **kw):
        out = sample_inner(*args, **kw)
        stats.append(dict(sampler.last_stats))
        return out
    sampler.sample_until_n_accepted = recording_sample
    abc = pa.ABCSMC(model, prior, dist, population_size=2000, sampler=sampler)
    abc.new("sqlite://", x0)
    append_inner = abc.history.append_population

    def recording_append(t, eps, population, *args, **kw):
        c = population.columns
        stored.append(dict(t=t, eps=float(eps), d=c.distances.clone(), x=c.sum_stats.clone(),
                           theta=c.theta.clone(), w=c.weights.clone()))
        return append_inner(t, eps, population, *args, **kw)
    abc.history.append_population = recording_append
    h = abc.run(max_nr_populations=3)
    assert h.max_t == 2
    return dict(dist=dist, keys=keys, x0=x0, updates=updates, stored=stored, stats=stats)


@pytest.fixture(scope="module")
def adaptive_runs(dev):
    return run_adaptive(True), run_adaptive(False)


def test_adaptive_run_stays_on_device(dev, adaptive_runs):
    from pyabc_amd import gpu
    from pyabc_amd.distance import SumStatMatrix
    run, _ = adaptive_runs
    keys, S = run["keys"], len(run["keys"])
    o = np.array([run["x0"][k] for k in keys])
    assert len(run["stats"]) >= 3
    for st in run["stats"]:
        assert not st.get("per_candidate", False), st
    assert len(run["updates"]) >= 3
    u53 = 2.0 ** -53
    for u in run["updates"]:
        assert isinstance(u["ss"], SumStatMatrix) and u["keys"] == keys
        assert u["ss"]._list is None
        X = u["seen"].cpu().numpy()
        assert X.shape[1] == S and X.shape[0] >= 2000
        dx = X - o
        terms = np.stack([np.abs(dx[:, :4]).sum(axis=1),
                          np.sqrt((dx[:, 4:] ** 2).sum(axis=1)),
                          np.abs(u["child_w"] * dx).max(axis=1)], axis=1)
        span = terms.max(axis=0) - terms.min(axis=0)
        # a term is a sum of at most S rounded quantities, here and on the
        # device: each within 2 S 2^-53 of the other, relative to the term
        # (the max is exact); the span of two such terms within that of the
        # largest one, twice
        tol = 2 * (2 * S * u53) * terms.max(axis=0) / span
        assert np.all(np.abs(u["scales"] - span) <= tol * span), (u["scales"], span)
    weights = run["dist"].weights
    for t, u in zip(sorted(weights), run["updates"]):
        same_bits(weights[t], 1 / u["scales"])
    x0d = gpu.as_dev(o)
    assert [s["t"] for s in run["stored"]] == [0, 1, 2]
    for s in run["stored"]:
        d = s["d"].cpu().numpy()
        again = run["dist"].device_call(s["x"], x0d, s["t"], keys).cpu().numpy()
        same_bits(d, again, f"t={s['t']}")
        assert d.shape == (2000,) and np.all(d <= s["eps"])


def test_adaptive_run_same_populations_without_the_tail(dev, adaptive_runs):
    run, plain = adaptive_runs
    assert len(run["stored"]) == len(plain["stored"]) == 3
    for a, b in zip(run["stored"], plain["stored"]):
        assert a["t"] == b["t"] and a["eps"] == b["eps"]
        for col in ("theta", "x", "d", "w"):
            same_bits(a[col].cpu().numpy().ravel(), b[col].cpu().numpy().ravel(),
                      f"t={a['t']} {col}")
