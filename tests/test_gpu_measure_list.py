"""The measure-list distances on the device: abc_whitened_norm,
abc_whitened_accept, abc_column_gram and abc_column_quantile against numpy,
the classes' device forms against the reference's values
(tests/golden/measure_list.npz) and ABCSMC runs on BatchedGPUSampler.

Every tolerance is worked out from the number format (u = 2^-53) and the
shape, next to its test.
"""
import logging

import numpy as np
import pytest

import measure_list_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = ref.U


@pytest.fixture(scope="module")
def dev():
    from pyabc_amd import gpu
    return gpu.require_device()


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture()


def same_bits(got, want, msg=""):
    """Equal as bit patterns, any NaN equal to any NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, msg
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=msg)
    np.testing.assert_array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64),
                                  err_msg=msg)


# ---- 1. abc_whitened_norm -------------------------------------------------------

def whiten_case(rng, B, S):
    """x [B, S] with a NaN entry (row 3) and an inf entry (row 5), x0 [S] and
    a random non-symmetric W [S, S]."""
    x = rng.normal(size=(B, S)) * 10.0 ** rng.uniform(-1, 1, size=S) + rng.normal(size=S)
    if B > 3:
        x[3, rng.integers(S)] = np.nan
    if B > 5:
        x[5, rng.integers(S)] = np.inf
    x0 = rng.normal(size=S)
    W = rng.normal(size=(S, S)) * 10.0 ** rng.uniform(-1, 1, size=(S, 1))
    return x, x0, W


@pytest.mark.parametrize("B", (1, 15, 16, 17, 1037))
@pytest.mark.parametrize("S", (1, 3, 4, 5, 16, 17, 64, 256))
def test_whitened_norm(dev, S, B):
    from pyabc_amd import gpu
    rng = np.random.default_rng(1000 * S + B)
    x, x0, W = whiten_case(rng, B, S)
    got = gpu.whitened_norm(gpu.as_dev(x), gpu.as_dev(x0), gpu.as_dev(W)).cpu().numpy()
    want, mag = ref.whitened(x, x0, W)
    fin = np.isfinite(want)
    assert fin.sum() >= B - 2
    # the dot-product bound: every output coordinate is a sum of S rounded
    # products of rounded differences, the norm a sum of S rounded squares
    # and a root: relative error (S + 4) u | |W| |x - x0| | / d
    err = np.abs(got[fin] - want[fin])
    print(f"S={S} B={B} max err / bound = {np.max(err / ((S + 4) * U * mag[fin])):.3f}")
    assert np.all(err <= (S + 4) * U * mag[fin])
    # plain IEEE: the NaN row is NaN, the inf row what numpy makes of it
    same_bits(got[~fin], want[~fin])
    if B > 5:
        assert np.isnan(got[3]) and np.isnan(want[3])
        assert got[5] == np.inf and want[5] == np.inf


def test_whitened_norm_not_transposed(dev):
    """An asymmetric W with one entry: W[i, j] maps statistic j to output i."""
    from pyabc_amd import gpu
    S = 20
    W = np.zeros((S, S))
    W[2, 17] = 3.0
    W[18, 1] = 0.5
    x = np.zeros((40, S))
    x[:, 17] = np.arange(40)
    x[:, 2] = 100.0
    x[:, 1] = 7.0
    got = gpu.whitened_norm(gpu.as_dev(x), gpu.as_dev(np.zeros(S)), gpu.as_dev(W)).cpu().numpy()
    same_bits(got, np.sqrt((3.0 * np.arange(40)) ** 2 + 3.5 ** 2))


def test_whitened_norm_empty(dev):
    from pyabc_amd import _native as nat, gpu
    # B = 0 returns before anything is read or launched
    assert nat.call("abc_whitened_norm", None, 0, 4, None, None, None, None) == 0
    out = gpu.whitened_norm(torch.empty((0, 4), dtype=torch.float64, device=dev),
                            gpu.as_dev(np.zeros(4)), gpu.as_dev(np.eye(4)))
    assert out.shape == (0,)
    with pytest.raises(ValueError):
        gpu.whitened_norm(gpu.as_dev(np.zeros((2, 257))), gpu.as_dev(np.zeros(257)),
                          gpu.as_dev(np.zeros((257, 257))))


# ---- 2. abc_whitened_accept ----------------------------------------------------

@pytest.mark.parametrize("B", (1, 63, 64, 65, 1037, 4133))
@pytest.mark.parametrize("S", (3, 17, 256))
def test_whitened_accept_equals_compact_of_the_distances(dev, S, B):
    from pyabc_amd import gpu
    rng = np.random.default_rng(77 * S + B)
    x, x0, W = whiten_case(rng, B, S)
    xd, x0d, Wd = gpu.as_dev(x), gpu.as_dev(x0), gpu.as_dev(W)
    d = gpu.whitened_norm(xd, x0d, Wd)
    dh = d.cpu().numpy()
    max_att = 50
    att = rng.integers(1, 40, size=B).astype(np.int32)
    att[rng.random(B) < 0.2] = max_att + 1 + rng.integers(0, 5)   # gave up
    attd = torch.from_numpy(att).to(dev)
    masked = gpu.mask_gave_up(d.clone(), attd, max_att)
    # eps is one row's exact distance (that row is accepted: d <= eps), the
    # median of the finite ones
    finite = np.sort(dh[np.isfinite(dh)])
    eps = float(finite[finite.size // 2]) if finite.size else 1.0
    for with_att in (False, True):
        widx, wcnt = gpu.accept_compact(masked if with_att else d, eps)
        n = int(wcnt.cpu()[0])
        want = widx.cpu().numpy()[:n]
        for cap in (B, max(n // 2, 1), 0):
            idx, cnt = gpu.whitened_accept(xd, x0d, Wd, eps, cap,
                                           att=attd if with_att else None,
                                           max_attempts=max_att)
            assert int(cnt.cpu()[0]) == n          # the count is not capped
            k = min(n, cap)
            np.testing.assert_array_equal(idx.cpu().numpy()[:k], want[:k])
    if finite.size:
        j = int(np.flatnonzero(dh == eps)[0])
        idx, cnt = gpu.whitened_accept(xd, x0d, Wd, eps, B)
        assert j in idx.cpu().numpy()[:int(cnt.cpu()[0])]


def test_whitened_accept_empty_round(dev):
    from pyabc_amd import gpu
    x = torch.empty((0, 5), dtype=torch.float64, device=dev)
    idx, cnt = gpu.whitened_accept(x, gpu.as_dev(np.zeros(5)), gpu.as_dev(np.eye(5)), 1.0, 10)
    assert int(cnt.cpu()[0]) == 0


# ---- 3. abc_column_gram ---------------------------------------------------------

@pytest.mark.parametrize("R,S", ((1, 1), (2, 2), (3, 5), (257, 17), (5000, 16), (300, 256)))
def test_column_gram(dev, R, S):
    from pyabc_amd import gpu
    rng = np.random.default_rng(31 * R + S)
    X = rng.normal(size=(R, S))
    if (R, S) in ((257, 17), (5000, 16)):
        X = X + 1e6          # a one-sweep sum of squares loses every digit here
    else:
        X = X * 10.0 ** rng.uniform(-1, 1, size=S) + rng.normal(size=S)
    Xd = gpu.as_dev(X)
    mean, G = gpu.column_gram(Xd)
    mean2, G2 = gpu.column_gram(Xd)
    mean, G = mean.cpu().numpy(), G.cpu().numpy()
    same_bits(G, G2.cpu().numpy())
    same_bits(mean, mean2.cpu().numpy())
    same_bits(G, G.T)
    m, Gl, absprod, abssum = ref.gram_longdouble(X)
    xmax = np.max(np.abs(X))
    # a sum of R values, whatever the order: within (R - 1) u max|X|, and one
    # division
    assert np.all(np.abs(mean - m) <= (R + 1) * U * xmax)
    # (R + 4) u sum_r |c_ri c_rj| for the R rounded products of rounded
    # differences and their sum; 2 u max|X| sum_r (|c_ri| + |c_rj|) for the
    # rounding of x - mean against the long-double centring
    bound = (R + 4) * U * absprod + 2 * U * xmax * (abssum[:, None] + abssum[None, :])
    err = np.abs(G - Gl).astype(np.float64)
    bound = bound.astype(np.float64)
    if R > 1:
        print(f"R={R} S={S} max err / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound)


# ---- 4. abc_column_quantile ------------------------------------------------------

QS = (0.0, 0.2, 0.5, 0.8, 1.0)
SMP = 4096      # abc_select.hip: sampled keys per column (R >= 4 SMP)


def quantile_matrix(rng, R, S):
    """Columns well away from zero (the tolerance is relative): random ones,
    and from S = 7 on a constant one, heavy ties, a sorted one, one whose
    evenly spaced sample misrepresents it, and one with a NaN."""
    X = rng.normal(size=(R, S)) * rng.uniform(0.5, 2.0, size=S) + rng.uniform(8.0, 12.0, size=S)
    kinds = {}
    if S >= 7:
        X[:, 1] = 4.25
        X[:, 2] = np.round(rng.normal(size=R) * 2.0) + 10.0
        X[:, 3] = np.sort(X[:, 3])
        # the sample takes rows ((2 q + 1) R) // (2 SMP): those alone are large
        pos = ((2 * np.arange(SMP) + 1) * R) // (2 * SMP)
        X[np.unique(pos), 4] += 1000.0
        X[R // 3, 5] = np.nan
        kinds = {1: "constant", 2: "ties", 3: "sorted", 4: "fallback", 5: "nan"}
    return X, kinds


@pytest.mark.parametrize("S", (1, 7, 256))
@pytest.mark.parametrize("R", (1, 2, 5, 16383, 16384, 70001))
def test_column_quantile(dev, R, S):
    from pyabc_amd import gpu
    rng = np.random.default_rng(13 * R + S)
    X, kinds = quantile_matrix(rng, R, S)
    Xd = gpu.as_dev(X)
    nan = np.isnan(X).any(axis=0)
    assert nan.sum() == (1 if S >= 7 else 0)
    with np.errstate(invalid="ignore"):
        want = np.percentile(X, [100 * q for q in QS], axis=0)
    for q, w in zip(QS, want):
        got = gpu.column_quantile(Xd, q).cpu().numpy()
        np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"q={q}")
        np.testing.assert_array_equal(np.isnan(w), nan)
        # the order statistics are exact: only the interpolation rounds (three
        # operations), relative to values no smaller than their spacing
        err = np.abs(got[~nan] - w[~nan]) / np.abs(w[~nan])
        assert np.all(err <= 1e-15), (q, np.max(err), np.argmax(err))
        if q in (0.0, 1.0):
            same_bits(got[~nan], (X.min(axis=0) if q == 0.0 else X.max(axis=0))[~nan])
        if q == 0.5:
            # every column is positive, so the median of |x - 0| is the
            # median pass abc_column_mad runs, on the same keys
            zero = torch.zeros(S, dtype=torch.float64, device=dev)
            med = gpu.column_scale(Xd, "mad_to_obs", zero).cpu().numpy()
            same_bits(got[~nan], med[~nan], "median")
            same_bits(got[~nan], np.median(X[:, ~nan], axis=0), "np.median")


def test_column_quantile_checks_arguments(dev):
    from pyabc_amd import gpu
    X = gpu.as_dev(np.ones((4, 3)))
    for q in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            gpu.column_quantile(X, q)


# ---- 5. the classes on the device ------------------------------------------------

def device_initialized(fx, name, tag, measures="all"):
    import pyabc_amd as pa
    from pyabc_amd import gpu
    from pyabc_amd.distance import SumStatMatrix
    cls = {"zscore": pa.ZScoreDistance, "pca": pa.PCADistance,
           "minmax": pa.MinMaxDistance, "percentile": pa.PercentileDistance}[name]
    sample = ref.sample_of(fx, tag[0])
    ks = ref.keys(sample.shape[1])
    x0 = dict(zip(ks, fx[f"{tag[0]}__x0"]))
    stats = SumStatMatrix(gpu.as_dev(sample), ks)
    dist = cls(measures_to_use=measures)
    dist.initialize(0, lambda: stats, x0)
    assert stats._list is None        # no list of dicts was made
    return dist, ks


@pytest.mark.parametrize("tag", ("A", "B", "C", "A_sub"))
@pytest.mark.parametrize("name", ("zscore", "pca", "minmax", "percentile"))
def test_classes_from_a_device_matrix(dev, fx, name, tag):
    from pyabc_amd import gpu
    sub = tag == "A_sub"
    measures = [f"y{k}" for k in fx["SUBSET"]] if sub else "all"
    dist, ks = device_initialized(fx, name, tag, measures)
    use = list(fx["SUBSET"]) if sub else list(range(len(ks)))
    if name == "minmax":
        same_bits([dist.normalization[k] for k in dist.measures_to_use],
                  fx[f"{tag}_minmax__norm"])
    if name == "percentile":
        got = np.array([dist.normalization[k] for k in dist.measures_to_use])
        want = fx[f"{tag}_percentile__norm"]
        assert np.all(np.abs(got - want) <= 1e-14 * np.abs(want))
    rows, x0 = fx[f"{tag[0]}__rows"], fx[f"{tag[0]}__x0"]
    d = dist.device_call(gpu.as_dev(rows), gpu.as_dev(x0), 0, ks).cpu().numpy()
    want = fx[f"{tag}_{name}__d"]
    if name == "pca":
        # first-order perturbation of G^(-1/2) under the Gram sum's rounding
        sample = ref.sample_of(fx, tag[0])
        tol = ref.cond2_gram(sample, use) * sample.shape[0] * U
    else:
        tol = 1e-12
    err = np.abs(d - want) / np.abs(want)
    print(f"{name} {tag}: max rel err {np.max(err):.3e} (tol {tol:.3e})")
    assert np.all(err <= tol)
    # the accept tail decides on device_call's bits
    tail = dist.accept_tail(0, ks, dev) if name == "pca" else \
        gpu.PNormTail(*dist.fused_pnorm(0, ks, dev))
    same_bits(tail.distances(gpu.as_dev(rows), gpu.as_dev(x0)).cpu().numpy(), d)


# ---- 6. end to end -------------------------------------------------------------------

E2E_S, E2E_N, E2E_GEN = 4, 500, 3


def run_e2e(name, accept_tail, zero_obs=False, pop=E2E_N, gens=E2E_GEN):
    import pyabc_amd as pa
    cls = {"zscore": pa.ZScoreDistance, "pca": pa.PCADistance,
           "minmax": pa.MinMaxDistance, "percentile": pa.PercentileDistance}[name]
    np.random.seed(3)
    names = ["t0", "t1"]
    keys = [f"s{k}" for k in range(E2E_S)]
    a = np.array([1.0, 0.7, 1.5, 0.4])
    sig = np.array([0.2, 0.5, 0.1, 1.0])
    x0 = dict(zip(keys, [0.8, -0.6, 1.1, 0.3]))
    if zero_obs:
        # statistic 1 is exactly 0 in every simulation and in the observation
        a[1] = sig[1] = 0.0
        x0["s1"] = 0.0
    model = pa.LinearGaussianModel(names, keys, src=np.arange(E2E_S) % 2, a=a, sigma=sig)
    prior = pa.Distribution(**{n: pa.RV("norm", 0, 1) for n in names})
    dist = cls()
    sampler = pa.BatchedGPUSampler(seed=5, allow_per_candidate=zero_obs,
                                   accept_tail=accept_tail)
    stats, stored = [], []
    inner = sampler.sample_until_n_accepted

    def recording_sample(*args, **kw):
        out = inner(*args, **kw)
        stats.append(dict(sampler.last_stats))
        return out
    sampler.sample_until_n_accepted = recording_sample
    abc = pa.ABCSMC(model, prior, dist, population_size=pop, sampler=sampler)
    abc.new("sqlite://", x0)
    append_inner = abc.history.append_population

    def recording_append(t, eps, population, *args, **kw):
        c = population.columns
        if c is not None:
            stored.append(dict(t=t, eps=float(eps), d=c.distances.cpu().numpy(),
                               x=c.sum_stats.cpu().numpy(), theta=c.theta.cpu().numpy(),
                               w=c.weights.cpu().numpy()))
        else:
            ps = population.get_list()
            stored.append(dict(t=t, eps=float(eps),
                               d=np.array([p.accepted_distances[0] for p in ps]),
                               x=np.array([[p.accepted_sum_stats[0][k] for k in keys]
                                           for p in ps])))
        return append_inner(t, eps, population, *args, **kw)
    abc.history.append_population = recording_append
    h = abc.run(max_nr_populations=gens)
    assert h.max_t == gens - 1
    return dict(dist=dist, keys=keys, x0=np.array([x0[k] for k in keys]), stats=stats,
                stored=stored)


@pytest.fixture(scope="module")
def e2e_runs(dev):
    return {}


def e2e(cache, name, tail):
    if (name, tail) not in cache:
        cache[(name, tail)] = run_e2e(name, tail)
    return cache[(name, tail)]


@pytest.mark.parametrize("name", ("zscore", "pca", "minmax", "percentile"))
def test_abcsmc_on_the_batched_sampler(dev, e2e_runs, name):
    run = e2e(e2e_runs, name, True)
    dist, o = run["dist"], run["x0"]
    # the calibration sample and the three generations, none per candidate
    gen_stats = run["stats"][-E2E_GEN:]
    assert len(run["stats"]) >= E2E_GEN
    for st in run["stats"]:
        assert not st.get("per_candidate", False), st
    for st in gen_stats:
        if name == "pca":
            assert not st.get("fused"), st      # staged rounds, whitened tail
        else:
            assert st.get("fused"), st          # the fused candidate round
    assert [s["t"] for s in run["stored"]] == list(range(E2E_GEN))
    use = range(E2E_S)
    for s in run["stored"]:
        assert s["d"].shape == (E2E_N,) and np.all(s["d"] <= s["eps"])
        if name == "pca":
            want, mag = ref.whitened(s["x"], o, dist._whitening_transformation_matrix)
            assert np.all(np.abs(s["d"] - want) <= (E2E_S + 4) * U * mag)
            continue
        if name == "zscore":
            want = ref.zscore(s["x"], o, use)
        else:
            want = ref.ranged(s["x"], o, [dist.normalization[k] for k in run["keys"]], use)
        assert np.all(np.abs(s["d"] - want) <= 1e-12 * want)


@pytest.mark.parametrize("name", ("zscore", "pca", "minmax", "percentile"))
def test_abcsmc_same_populations_without_the_tail(dev, e2e_runs, name):
    run, plain = e2e(e2e_runs, name, True), e2e(e2e_runs, name, False)
    assert len(run["stored"]) == len(plain["stored"]) == E2E_GEN
    for a, b in zip(run["stored"], plain["stored"]):
        assert a["t"] == b["t"] and a["eps"] == b["eps"]
        for col in ("theta", "x", "d", "w"):
            same_bits(a[col].ravel(), b[col].ravel(), f"t={a['t']} {col}")


def test_zscore_zero_observation_takes_the_per_candidate_loop(dev, caplog):
    with caplog.at_level(logging.WARNING):
        run = run_e2e("zscore", True, zero_obs=True, pop=30, gens=2)
    assert any(st.get("per_candidate") for st in run["stats"])
    assert "ZScoreDistance with a zero observation" in caplog.text
    o = run["x0"]
    for s in run["stored"]:
        assert np.all(s["x"][:, 1] == 0.0)
        want = (np.abs((s["x"][:, [0, 2, 3]] - o[[0, 2, 3]]) / o[[0, 2, 3]])).sum(axis=1) / 4
        assert np.all(np.abs(s["d"] - want) <= 1e-12 * want) and np.all(s["d"] <= s["eps"])
