"""Integer parameters on the device: grid priors and the discrete random
walk (pyabc_amd/csrc/abc_walk.hip) against the numpy replay and the exact
rational mass of tests/walk_ref.py, and the batched sampler over them."""
import math

import numpy as np
import pandas as pd
import pytest
import scipy.stats as st

import walk_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _spec(frozen):
    import pyabc_amd as pa
    rv = pa.RV("poisson", 1)
    rv.distribution = frozen
    spec, why = rv.grid_spec()
    assert spec is not None, why
    return spec


def _law(n, p_l, p_r, p_c):
    from pyabc_amd.transition.randomwalk import walk_step_law
    return walk_step_law(n, p_l, p_r, p_c)


# ---- grid prior ------------------------------------------------------------------

GRIDS = {
    1: lambda: [_spec(st.poisson(3))],
    # a table with an interior entry of mass 0, a bounded and a shifted one
    3: lambda: [_spec(st.rv_discrete(values=([0, 2, 5], [.25, .5, .25]))(loc=-1)),
                _spec(st.binom(50, .3)), _spec(st.poisson(3, loc=-2))],
}


@pytest.mark.parametrize("d", [1, 3])
def test_grid_prior_draw_and_logpmf_equal_the_replay(d):
    from pyabc_amd import gpu
    spec = GRIDS[d]()
    prior = gpu.GridPrior(spec)
    B, idx0 = 1000, 2 ** 32 - 500       # crosses the index word's 32-bit boundary
    theta = prior.draw(seed=77, generation=3, idx0=idx0, B=B)
    want = walk_ref.grid_draw(spec, 77, 3, idx0, B)
    assert np.array_equal(theta.cpu().numpy(), want)
    lp = prior.logpmf_rows(theta).cpu().numpy()
    assert np.array_equal(lp, walk_ref.grid_logpmf(want, spec))
    assert np.isfinite(lp).all()         # every draw has positive mass
    for k, (k_lo, pmf, _) in enumerate(spec):
        assert len(np.unique(want[:, k])) > 1
    # edges, holes, fractions
    base = np.array([[s[0] for s in spec]], dtype=np.float64)      # every k_lo
    rows = [base[0].copy()]
    for k, (k_lo, pmf, _) in enumerate(spec):
        for v in (k_lo - 1, k_lo + len(pmf), k_lo + len(pmf) - 1, k_lo + 0.5, np.nan,
                  np.inf, -1e300):
            r = base[0].copy()
            r[k] = v
            rows.append(r)
        for hole in np.nonzero(np.asarray(pmf) == 0)[0]:
            r = base[0].copy()
            r[k] = k_lo + hole
            rows.append(r)
    if d == 3:
        rows.append(np.array([-2.0, 0.5, 0.0]))     # outside and a fraction: NaN
    rows = np.array(rows)
    got = prior.logpmf_rows(gpu.as_dev(rows)).cpu().numpy()
    want = walk_ref.grid_logpmf(rows, spec)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isfinite(got[0])
    assert got[1] == -np.inf and got[2] == -np.inf and np.isfinite(got[3])
    assert np.isnan(got[4]) and np.isnan(got[5]) and got[6] == -np.inf and got[7] == -np.inf
    if d == 3:
        assert (np.asarray(spec[0][1]) == 0).sum() == 3       # the holes were tested
        assert np.isnan(got[-1])


# ---- proposals ------------------------------------------------------------------

def _dyadic_weights(rng, N):
    """Multiples of 2^-10 summing to 1: every partial sum is exact, so the
    device scan and numpy's cumsum hold the same bits."""
    if N == 1:
        return np.array([1.0])
    m = rng.multinomial(1024, np.full(N, 1.0 / N))
    return m / 1024.0


def _device_population(X, w):
    from pyabc_amd import gpu
    Xd, wd = gpu.as_dev(np.asarray(X, dtype=np.float64)), gpu.as_dev(w)
    Xi, bad = gpu.walk_pack(Xd)
    assert int(bad.item()) == 0
    assert np.array_equal(Xi.cpu().numpy(), np.asarray(X, dtype=np.int32))
    cdf = gpu.inclusive_scan(wd)
    assert np.array_equal(cdf.cpu().numpy(), np.cumsum(w))
    return Xd, wd, Xi, cdf, gpu.cdf_guide(cdf)


def _propose(X, w, law, seed, gen, idx0, B, spec=None, max_attempts=1, use_guide=True):
    from pyabc_amd import gpu
    _, _, Xi, cdf, guide = _device_population(X, w)
    n = (len(law) - 1) // 2
    prior = None if spec is None else gpu.GridPrior(spec)
    out = gpu.walk_propose(Xi, cdf, guide if use_guide else None,
                           gpu.as_dev(np.cumsum(law)), n, walk_ref.last_positive(law),
                           seed, gen, idx0, B, max_attempts, prior)
    return [t.cpu().numpy() for t in out]


WALKS = [(1, 1. / 3, 1. / 3, 1. / 3), (7, .2, .5, .3), (4, .5, .5, 0.)]


@pytest.mark.parametrize("setting", WALKS, ids=["n1", "n7", "n4_pc0"])
@pytest.mark.parametrize("N", [1, 100])
@pytest.mark.parametrize("d", [1, 2, 3, 5, 32])
def test_walk_propose_equals_the_replay(d, N, setting):
    rng = np.random.default_rng(1000 * d + N)
    X = rng.integers(-50, 50, size=(N, d))
    w = _dyadic_weights(rng, N)
    law = _law(*setting)
    B, idx0 = 500, 2 ** 32 - 250
    theta, lp, anc, att = _propose(X, w, law, 5, 2, idx0, B, use_guide=(d != 3))
    rt, rl, ra, ratt = walk_ref.walk_propose(X, w, law, 5, 2, idx0, B)
    assert np.array_equal(anc, ra)
    assert np.array_equal(theta, rt)
    assert np.array_equal(att, ratt) and (att == 1).all()
    assert np.array_equal(lp, rl)               # no prior: log mass 0
    s = theta - X[anc]
    assert np.abs(s).max() <= setting[0]
    if N > 1:
        assert len(np.unique(anc)) > 10 and (w[anc] > 0).all()
    if setting[3] == 0.0:
        assert ((s.astype(np.int64) - setting[0]) % 2 == 0).all()   # parity gaps never drawn
    assert len(np.unique(s)) > 1


def test_walk_propose_redraws_outside_the_prior():
    """randint(0, 4) on both coordinates, the population on its edges: part
    of the proposals leave the prior and are drawn again, as the replay does."""
    rng = np.random.default_rng(8)
    spec = [_spec(st.randint(0, 4)), _spec(st.randint(0, 4))]
    X = rng.choice([0, 3], size=(100, 2))
    w = _dyadic_weights(rng, 100)
    law = _law(2, 1. / 3, 1. / 3, 1. / 3)
    B, idx0 = 1000, 123456789
    theta, lp, anc, att = _propose(X, w, law, 9, 1, idx0, B, spec, max_attempts=50)
    rt, rl, ra, ratt = walk_ref.walk_propose(X, w, law, 9, 1, idx0, B, spec, 50)
    assert np.array_equal(theta, rt) and np.array_equal(anc, ra)
    assert np.array_equal(att, ratt) and np.array_equal(lp, rl)
    assert (att >= 2).sum() > 100 and att.max() <= 50
    assert ((theta >= 0) & (theta <= 3)).all() and np.isfinite(lp).all()


def test_walk_propose_gives_up_after_max_attempts():
    spec = [_spec(st.randint(0, 4))] * 2
    X = np.full((5, 2), 100)
    w = np.array([.25, .25, .25, .125, .125])
    law = _law(2, 1. / 3, 1. / 3, 1. / 3)
    theta, lp, anc, att = _propose(X, w, law, 9, 1, 0, 300, spec, max_attempts=3)
    rt, rl, ra, ratt = walk_ref.walk_propose(X, w, law, 9, 1, 0, 300, spec, 3)
    assert (att == 4).all() and (lp == -np.inf).all()
    assert np.array_equal(theta, rt) and np.array_equal(anc, ra) and np.array_equal(att, ratt)


# ---- density ----------------------------------------------------------------------

TILE = 256
# (N, M, d, n_steps): every N, M, d and n of the list appears; N = TILE + 1 is
# one tile and a row, 769 and 1025 make at least 3 chunks
DENSITY = [(1, 1, 1, 1), (63, 257, 2, 7), (64, 1, 8, 1), (65, 257, 9, 7),
           (TILE + 1, 257, 5, 7), (769, 257, 2, 1), (769, 1, 32, 512),
           (TILE + 1, 1, 9, 512), (65, 257, 32, 1), (1025, 257, 8, 7),
           (64, 257, 1, 512), (63, 1, 32, 7), (1025, 1, 1, 1)]


def _density_case(N, M, d, n, seed):
    """A population spread so that about 4000 pairs lie within n in every
    coordinate, candidates next to particles (so their mass is far above the
    underflow threshold) plus some far from every particle."""
    rng = np.random.default_rng(seed)
    frac = min(1.0, 4000.0 / (M * N))
    W = int(math.ceil((2 * n + 1) / frac ** (1.0 / d)))
    X = rng.integers(0, W, size=(N, d))
    w = rng.random(N) + 0.1
    if N > 2:
        w[rng.integers(0, N, size=max(1, N // 8))] = 0.0      # some w_j = 0
        w[0] = 0.7
    w /= w.sum()
    near = min(n, 3)
    x = X[rng.integers(0, N, size=M)] + rng.integers(-near, near + 1, size=(M, d))
    if M > 3:
        x[-3:] += 10 ** 6                # far from every particle: exactly -inf
    return X, w, x


@pytest.mark.parametrize("N,M,d,n", DENSITY)
def test_walk_logpmf_against_exact_mass(N, M, d, n):
    from pyabc_amd import gpu
    X, w, x = _density_case(N, M, d, n, 31 * N + M + d + n)
    law = _law(n, .3, .45, .25)
    Xd, wd, Xi, _, _ = _device_population_any(X, w)
    chunk = gpu.walk_logpmf_chunk(M, N, d)
    assert chunk % TILE == 0
    if N >= 769:
        assert -(-N // chunk) >= 3
    xd = gpu.as_dev(x.astype(np.float64))
    out = gpu.walk_logpmf(xd, Xi, wd, gpu.as_dev(law), n)
    again = gpu.walk_logpmf(xd, Xi, wd, gpu.as_dev(law), n)
    assert gpu.torch.equal(out, again)                  # same bits on every call
    got = out.cpu().numpy()
    exact = walk_ref.exact_mass(x, X, w, law)
    want = np.array([walk_ref.log_fraction(f) for f in exact])
    tol = (N + d + 8) * U + 4 * U * np.abs(np.where(np.isfinite(want), want, 0.0))
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin])        # exactly -inf
    err = np.abs(got[fin] - want[fin])
    print(f"N={N} M={M} d={d} n={n}: max err {err.max() if fin.any() else 0:.3g}, "
          f"bound {tol[fin].min() if fin.any() else 0:.3g}")
    assert (err <= tol[fin]).all(), (err.max(), tol[fin].min())
    assert fin.any()


def _device_population_any(X, w):
    """Like _device_population for weights whose scan need not be exact."""
    from pyabc_amd import gpu
    Xd, wd = gpu.as_dev(np.asarray(X, dtype=np.float64)), gpu.as_dev(w)
    Xi, bad = gpu.walk_pack(Xd)
    assert int(bad.item()) == 0
    return Xd, wd, Xi, None, None


def test_walk_logpmf_far_fraction_and_cap():
    """Candidates far from every particle give exactly -inf, a fraction or a
    NaN gives NaN, coordinates at +-2^30 are handled exactly, values beyond
    the int32 range are far."""
    from pyabc_amd import gpu
    C = 2 ** 30
    X = np.array([[C, -C], [C - 1, -C + 2], [0, 0], [5, 5]])
    w = np.array([.25, .25, .125, .375])
    n = 2
    law = _law(n, .25, .25, .5)
    x = np.array([[C, -C], [C - 2, -C + 1], [C, -C + 4], [1, -1], [4, 7],
                  [0, 3], [2 ** 31 + 7, 0], [-1e18, 0], [1e300, -1e300], [np.inf, 0],
                  [0.5, 0], [0, np.nan], [3 * C, 0.5]], dtype=np.float64)
    _, wd, Xi, _, _ = _device_population_any(X, w)
    got = gpu.walk_logpmf(gpu.as_dev(x), Xi, wd, gpu.as_dev(law), n).cpu().numpy()
    exact = walk_ref.exact_mass(x[:6], X, w, law)
    want = np.array([walk_ref.log_fraction(f) for f in exact])
    assert np.isfinite(want[:5]).all() and want[5] == -np.inf
    tol = (4 + 2 + 8) * U + 4 * U * np.abs(want[:5])
    assert (np.abs(got[:5] - want[:5]) <= tol).all()
    assert (got[5:10] == -np.inf).all()
    assert np.isnan(got[10:]).all()
    # the pack refuses what the kernels cannot hold
    for bad_value in (0.5, np.nan, C + 1.0, -np.inf):
        Xb = X.astype(np.float64)
        Xb[2, 1] = bad_value
        _, bad = gpu.walk_pack(gpu.as_dev(Xb))
        assert int(bad.item()) == 1


def test_fit_device_raises_on_a_fraction():
    import pyabc_amd as pa
    from pyabc_amd import gpu
    X = np.array([[1.0, 2.0], [3.0, 0.5], [2.0, 2.0]])
    tr = pa.DiscreteRandomWalkTransition()
    with pytest.raises(ValueError, match="can only handle integer values"):
        tr.fit_device(gpu.as_dev(X), gpu.as_dev(np.full(3, 1 / 3)), ["a", "b"])


def test_transition_device_form_equals_host_form():
    """fit_device: pdf and rvs run the kernels; a host fit stays numpy and
    logpdf_device uploads it on first use."""
    import pyabc_amd as pa
    from pyabc_amd import gpu
    rng = np.random.default_rng(4)
    X = pd.DataFrame(rng.integers(0, 6, size=(50, 2)).astype(float), columns=["a", "b"])
    w = rng.random(50)
    w /= w.sum()
    x = pd.DataFrame(rng.integers(-1, 8, size=(40, 2)).astype(float), columns=["a", "b"])
    host = pa.DiscreteRandomWalkTransition(n_steps=2)
    host.fit(X, w.copy())
    assert getattr(host, "_dev_X", None) is None
    want = host.pdf(x)
    dev = pa.DiscreteRandomWalkTransition(n_steps=2)
    dev.fit_device(gpu.as_dev(X.values), gpu.as_dev(w), ["a", "b"])
    assert dev._dev_Xi is not None and dev._dev_cdf is not None and dev._dev_guide is not None
    got = dev.pdf(x)
    assert np.array_equal(got == 0, want == 0)
    np.testing.assert_allclose(got, want, rtol=1e-13)
    assert dev.pdf(x.iloc[0]) == pytest.approx(want[0], rel=1e-13)
    draws = dev.rvs(200)
    assert list(draws.columns) == ["a", "b"] and np.array_equal(draws.values, np.rint(draws.values))
    assert (dev.pdf(draws) > 0).all()
    with pytest.raises(ValueError):
        dev.pdf(pd.DataFrame([[0.5, 1.0]], columns=["a", "b"]))
    # lazily uploaded after a host fit
    lazy = gpu.torch.exp(host.logpdf_device(gpu.as_dev(x.values))).cpu().numpy()
    np.testing.assert_allclose(lazy, want, rtol=1e-13)
    # over the kernels' limits: the host form stays
    big = pa.DiscreteRandomWalkTransition(n_steps=600)
    big.fit_device(gpu.as_dev(X.values), gpu.as_dev(w), ["a", "b"])
    assert getattr(big, "_dev_X", None) is None and len(big.X) == 50


# ---- the sampler --------------------------------------------------------------------

def _s64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def _noise(shape_like, seed, gen, idx0):
    """Standard normals keyed by (seed, generation, global candidate index,
    column) alone (a splitmix64 hash in wrapping int64 arithmetic, then the
    inverse normal CDF): the same value whatever the round's size."""
    import torch
    B, S = shape_like.shape
    dev = shape_like.device
    g = idx0 + torch.arange(B, dtype=torch.int64, device=dev)[:, None]
    col = torch.arange(S, dtype=torch.int64, device=dev)[None, :]
    x = g * _s64(0x9E3779B97F4A7C15) + col * _s64(0xD1B54A32D192ED03) \
        + _s64(seed * 1000003 + gen * 7919 + 12345)
    x = (x ^ ((x >> 30) & ((1 << 34) - 1))) * _s64(0xBF58476D1CE4E5B9)
    x = (x ^ ((x >> 27) & ((1 << 37) - 1))) * _s64(0x94D049BB133111EB)
    x = x ^ ((x >> 31) & ((1 << 33) - 1))
    u = (((x >> 12) & ((1 << 52) - 1)).to(torch.float64) + 0.5) * 2.0 ** -52
    return math.sqrt(2.0) * torch.erfinv(2.0 * u - 1.0)


SIGMA = 0.5


def _run(prior, keys, x0, batch_size, pop=2000, gens=4, seed=11):
    import pyabc_amd as pa
    names = prior.get_parameter_names()

    def sim(theta, seed, gen, idx0):
        return theta[:, :len(keys)] + SIGMA * _noise(theta[:, :len(keys)], seed, gen, idx0)

    sampler = pa.BatchedGPUSampler(seed=seed, allow_per_candidate=False,
                                   batch_size=batch_size)
    abc = pa.ABCSMC(pa.VectorizedModel(sim, keys), prior, pa.PNormDistance(p=2),
                    population_size=pop, sampler=sampler,
                    transitions=pa.DiscreteRandomWalkTransition(n_steps=2),
                    eps=pa.MedianEpsilon())
    abc.new("sqlite://", x0)
    stats = []
    sampler_hook = sampler.sample_until_n_accepted

    def wrapped(*a, **k):
        out = sampler_hook(*a, **k)
        stats.append(dict(sampler.last_stats))
        return out
    sampler.sample_until_n_accepted = wrapped
    h = abc.run(max_nr_populations=gens)
    assert h.max_t == gens - 1
    assert stats and not any(s.get("per_candidate") for s in stats)
    pops = [h.get_distribution(0, t) for t in range(gens)]
    eps = h.get_all_populations().query("t >= 0").sort_values("t")["epsilon"].to_numpy()
    return names, pops, eps


def _check_weights(prior, names, pops):
    """w_t = prior.pmf / transition.pdf, recomputed on the host from the
    previous generation and normalised."""
    import pyabc_amd as pa
    for t in range(1, len(pops)):
        (dfp, wp), (df, w) = pops[t - 1], pops[t]
        tr = pa.DiscreteRandomWalkTransition(n_steps=2)
        tr.fit(dfp[names], np.asarray(wp, dtype=np.float64).copy())
        assert getattr(tr, "_dev_X", None) is None        # the numpy form
        pm = np.ones(len(df))
        for nm in names:
            pm = pm * prior[nm].pmf(df[nm].to_numpy())
        ref = pm / tr.pdf(df[names])
        np.testing.assert_allclose(w, ref / ref.sum(), rtol=1e-11, atol=0)


@pytest.fixture(scope="module")
def poisson_run():
    import pyabc_amd as pa
    prior = pa.Distribution(k=pa.RV("poisson", 3))
    return prior, _run(prior, ["y"], {"y": 4.0}, batch_size=4096)


def test_sampler_poisson_prior_stays_batched(poisson_run):
    prior, (names, pops, eps) = poisson_run
    for df, w in pops:
        k = df["k"].to_numpy()
        assert len(k) == 2000 and np.array_equal(k, np.rint(k))
        assert (prior["k"].pmf(k) > 0).all()
        assert (w > 0).all() and abs(w.sum() - 1) < 1e-12
    _check_weights(prior, names, pops)
    assert (np.diff(eps) < 0).all()


def test_sampler_posterior_matches_exact_abc_posterior(poisson_run):
    prior, (names, pops, eps) = poisson_run
    df, w = pops[-1]
    e, y0 = eps[-1], 4.0
    ks = np.arange(0, 60)
    post = st.poisson(3).pmf(ks) * (st.norm.cdf((y0 + e - ks) / SIGMA)
                                    - st.norm.cdf((y0 - e - ks) / SIGMA))
    post /= post.sum()
    ess = 1.0 / np.sum(np.asarray(w) ** 2)
    bins = ks[post >= 0.01]
    assert len(bins) >= 3
    for k in bins:
        got = float(np.sum(w[df["k"].to_numpy() == k]))
        se = math.sqrt(post[k] * (1 - post[k]) / ess)
        print(f"k={k}: weighted {got:.4f}, exact {post[k]:.4f}, {abs(got - post[k]) / se:.2f} se")
        assert abs(got - post[k]) <= 5 * se, (k, got, post[k], se)


def test_sampler_round_size_does_not_change_the_population(poisson_run):
    import pyabc_amd as pa
    prior, (names, pops, eps) = poisson_run
    _, small, eps_small = _run(pa.Distribution(k=pa.RV("poisson", 3)), ["y"], {"y": 4.0},
                               batch_size=64)
    assert np.array_equal(eps, eps_small)
    for (df, w), (df2, w2) in zip(pops, small):
        assert np.array_equal(df.to_numpy(), df2.to_numpy())
        assert np.array_equal(np.asarray(w), np.asarray(w2))


def test_sampler_two_discrete_parameters():
    import pyabc_amd as pa
    prior = pa.Distribution(a=pa.RV("binom", 10, .4), b=pa.RV("randint", 0, 4))
    names, pops, eps = _run(prior, ["y0", "y1"], {"y0": 5.0, "y1": 2.0}, batch_size=None)
    assert names == ["a", "b"]
    for df, w in pops:
        v = df[names].to_numpy()
        assert np.array_equal(v, np.rint(v))
        assert (prior["a"].pmf(v[:, 0]) > 0).all() and (prior["b"].pmf(v[:, 1]) > 0).all()
        assert (w > 0).all()
    _check_weights(prior, names, pops)


def test_generation_spec_is_batched_capable_with_a_grid_prior():
    import pyabc_amd as pa
    prior = pa.Distribution(k=pa.RV("poisson", 3))
    abc = pa.ABCSMC(pa.VectorizedModel(lambda th, s, g, i: th, ["y"]), prior,
                    pa.PNormDistance(p=2), population_size=50,
                    sampler=pa.BatchedGPUSampler(),
                    transitions=pa.DiscreteRandomWalkTransition())
    abc.x_0 = {"y": 0.0}
    spec = pa.GenerationSpec(abc, 0)
    assert spec.batched_capable and spec.why_not == "" and spec.grid is not None
    assert spec.grid_prior.d == 1 and prior.device_spec() is None


# ---- AdaptivePopulationSize's bootstrap ------------------------------------------

@pytest.mark.parametrize("n_boot", [100, 300])
def test_mean_cv_runs_the_device_bootstrap(n_boot, monkeypatch):
    import pyabc_amd as pa
    from pyabc_amd import gpu
    from pyabc_amd.cv import bootstrap

    def no_host(*a, **k):
        raise AssertionError("the host bootstrap ran")
    monkeypatch.setattr(bootstrap, "_model_cv_host", no_host)
    rng = np.random.default_rng(6)
    X = rng.integers(0, 4, size=(300, 2)).astype(np.float64)
    w = rng.random(300) + 0.5
    w /= w.sum()
    tr = pa.DiscreteRandomWalkTransition(n_steps=1)
    tr.fit_device(gpu.as_dev(X), gpu.as_dev(w), ["a", "b"])
    assert bootstrap._is_device(tr)
    np.random.seed(2)
    cv = tr.mean_cv(n_boot)
    var = np.asarray(tr.variation_at_test_points_)
    assert var.shape == (300,)
    assert np.isfinite(var).all() and (var > 0).all()
    assert np.isfinite(cv) and cv > 0
