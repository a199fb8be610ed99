"""The drop-in's fallbacks on the GPU engine.

* A prior component without a device sampler (any scipy family besides the
  seven kernel families) takes the host-scipy leg: its support interval goes
  to the device (re-draw test), its t = 0 draws are scipy's ppf of the
  candidates' own prior-stream uniforms, and its density multiplies into the
  importance weights on the host (random_variables.py:111-196, 412-452).
* A closure the batched kernels cannot run (a plain per-particle model)
  goes through the reference's per-candidate loop inside BatchedGPUSampler
  (sampler/base.py:172-214, singlecore.py:20-38).

Parity: the host leg's draws against scipy's ppf of the oracle's replay of
the uniforms (exact), and whole generations' importance weights against the
oracle's prior / transition density (smc.py:768-811) on the populations the
engine produced (2e-6 relative: the hinted x3 density's bar).
"""
import os

import numpy as np
import pandas as pd
import pytest
from scipy import stats

import oracle
import oracle.sampler as osamp
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _weights_vs_oracle(h, prior_logpdf, rtol=2e-6):
    """Every generation t >= 1: w_t ∝ prior(x) / sum_j w_j N(x - X_j; Sigma)
    with (X, w) the population of t - 1 and Sigma its MVN fit."""
    checked = 0
    for t in range(1, h.max_t + 1):
        dfp, wp = h.get_distribution(0, t - 1)
        df, w = h.get_distribution(0, t)
        cols = sorted(df.columns)
        Xp, x = dfp[cols].to_numpy(), df[cols].to_numpy()
        cov, wpn = oracle.mvn_fit(Xp, wp)
        lt = oracle.mvn_logpdf(x, Xp, wpn, cov)
        lw = prior_logpdf(x) - lt
        ref = np.exp(lw - lw.max())
        ref /= ref.sum()
        np.testing.assert_allclose(w, ref, rtol=rtol, atol=0)
        checked += 1
    assert checked >= 1


def test_host_prior_draws_replay():
    """t = 0 draws of host-leg coordinates: ppf(u) of the candidates' prior
    uniforms, u replayed by the oracle; device-family coordinates untouched;
    the host coordinates' support intervals reach the device."""
    import pyabc_amd as pa
    from pyabc_amd import gpu
    from pyabc_amd.random_variables import host_prior_draw
    prior = pa.Distribution(a=pa.RV("t", 3), b=pa.RV("norm", 1, 2),
                            c=pa.RV("triang", 0.5, -1, 3))
    from pyabc_amd._native import PRIOR_KINDS as K
    kinds, params = prior.device_spec()
    assert list(kinds) == [K["host"], K["norm"], K["host"]]
    np.testing.assert_array_equal(params.reshape(3, 4)[2, :3], [-1.0, 2.0, 0.5])
    host = prior.host_components()
    assert [c for c, _ in host] == [0, 2]
    dev = gpu.require_device()
    seed, gen, lo, B = 4242, 0, 1_000_003, 50_000
    th, lp, _, att = gpu.propose(None, None, None, gpu.as_dev(kinds, dtype=torch.int32),
                                 gpu.as_dev(params), seed, gen, lo, B, 100, 3)
    before = th[:, 1].clone()
    host_prior_draw(th, att, host, seed, gen, lo)
    assert torch.equal(th[:, 1], before)
    idx = np.arange(lo, lo + B, dtype=np.uint64)
    a = att.cpu().numpy()
    for col, rv in host:
        u = osamp.prior_uniforms(idx, a, col, gen, seed)
        np.testing.assert_array_equal(th[:, col].cpu().numpy(), rv.distribution.ppf(u))
    got = th.cpu().numpy()
    assert ((got[:, 2] >= -1) & (got[:, 2] <= 2)).all()
    # the draws follow the priors (KS at alpha 1e-3)
    assert stats.kstest(got[:, 0], stats.t(3).cdf).pvalue > 1e-3
    assert stats.kstest(got[:, 2], stats.triang(0.5, -1, 3).cdf).pvalue > 1e-3


def test_host_prior_leg_in_generations():
    """ABCSMC with a vectorised model and a prior mixing device families with
    scipy's t and triang: calibration and t = 0 on the staged path (host
    draws), later generations on the fused rounds (device support test);
    every generation's weights equal the oracle's prior / transition."""
    import pyabc_amd as pa
    names = ["a", "b", "c"]
    prior = pa.Distribution(a=pa.RV("t", 3), b=pa.RV("norm", 0, 1),
                            c=pa.RV("triang", 0.5, -1, 3))
    model = pa.LinearGaussianModel(names, ["y0", "y1", "y2"], src=[0, 1, 2],
                                   sigma=[0.5] * 3)
    sampler = pa.BatchedGPUSampler(seed=5)
    abc = pa.ABCSMC(model, prior, pa.PNormDistance(p=2), population_size=4000,
                    sampler=sampler, eps=pa.QuantileEpsilon(alpha=0.5))
    abc.new("sqlite://", {"y0": 1.0, "y1": 0.5, "y2": 0.8})
    fused = []
    abc.generation_callback = lambda t: fused.append(bool(sampler.last_stats.get("fused")))
    h = abc.run(max_nr_populations=4)
    assert h.max_t == 3
    assert fused == [False, True, True, True]

    def prior_lp(x):
        return (stats.t(3).logpdf(x[:, 0]) + stats.norm.logpdf(x[:, 1])
                + stats.triang(0.5, -1, 3).logpdf(x[:, 2]))
    _weights_vs_oracle(h, prior_lp)
    for t in range(h.max_t + 1):
        df, _ = h.get_distribution(0, t)
        assert ((df["c"] >= -1) & (df["c"] <= 2)).all()


def test_plain_model_per_candidate_loop():
    """ABCSMC(scalar_model, Distribution(x=RV("t", 3)), ...,
    sampler=BatchedGPUSampler()): the per-particle model cannot run batched,
    so the sampler loops over simulate_one (the reference's sampler
    contract); the transition density of each accepted particle still runs
    on the device.  Weights vs the oracle, and a check_max_eval stop."""
    import pyabc_amd as pa
    np.random.seed(11)

    def model(p):
        return {"y": p["x"] + 0.5 * np.random.randn()}
    sampler = pa.BatchedGPUSampler()
    abc = pa.ABCSMC(model, pa.Distribution(x=pa.RV("t", 3)), pa.PNormDistance(),
                    population_size=300, sampler=sampler)
    abc.new("sqlite://", {"y": 1.0})
    h = abc.run(max_nr_populations=3)
    assert h.max_t == 2
    assert sampler.last_stats.get("per_candidate")
    assert sampler.nr_evaluations_ >= 300
    _weights_vs_oracle(h, lambda x: stats.t(3).logpdf(x[:, 0]))
    # max_eval stop (singlecore.py:25-31 semantics)
    s2 = pa.BatchedGPUSampler(check_max_eval=True)
    sample = s2.sample_until_n_accepted(50, lambda: pa.Particle(
        m=0, parameter=pa.Parameter(x=0.0), weight=1.0, accepted_sum_stats=[],
        accepted_distances=[], accepted=False), max_eval=40)
    assert not sample.ok and s2.nr_evaluations_ == 40


@pytest.mark.parametrize("d,N,k", [(20, 1500, None), (17, 700, 40), (33, 400, None),
                                   (80, 400, None), (72, 300, 90)])
def test_local_transition_wide_vs_oracle(d, N, k):
    """LocalTransition above d = 16 (the reference has no dimension cap,
    local_transition.py:77-96): the runtime-d fit, density and proposal
    against the oracle -- covariances, inverses, determinants and densities
    to 1e-9 relative, proposals replayed to 1e-12.  d = 72, 80: the BIG path
    (per-particle matrices in the workspace, the wide propose kernel)."""
    import pyabc_amd as pa
    rng = np.random.default_rng(d + N)
    A = rng.normal(size=(d, d)) / np.sqrt(d)
    X = rng.normal(size=(N, d)) @ A.T + np.where(rng.uniform(size=(N, 1)) < 0.5, 1.5, -1.0)
    w = np.exp(0.5 * rng.standard_normal(N))
    w /= w.sum()
    cols = [f"p{q:02d}" for q in range(d)]
    tr = pa.LocalTransition(k=k, k_fraction=None) if k else pa.LocalTransition()
    tr.fit(pd.DataFrame(X, columns=cols), w.copy())
    ref = oracle.local_fit(X, w, k=k, k_fraction=None if k else 0.25)
    assert tr.k == ref["k"]
    np.testing.assert_allclose(tr.covs, ref["covs"], rtol=1e-9, atol=1e-13)
    # inverses and determinants amplify the covariances' last-bit
    # differences by the condition number (a 33-D covariance of 100
    # neighbours is poorly conditioned): compared matrix-wise, relative to
    # each inverse's largest entry
    inv, inv_ref = tr.inv_covs, ref["inv_covs"]
    scale = np.abs(inv_ref).max(axis=(1, 2))
    assert (np.abs(inv - inv_ref).max(axis=(1, 2)) <= 1e-8 * scale).all()
    np.testing.assert_allclose(tr.determinants, ref["dets"], rtol=1e-7)
    x = X[rng.integers(0, N, 300)] + 0.05 * rng.standard_normal((300, d))
    got = np.log(tr.pdf(pd.DataFrame(x, columns=cols)))
    want = np.log(oracle.local_pdf(x, X, ref))
    # log densities: the quadratic forms reach ~1e3 in 33-D, where the
    # inverses' conditioning shows; 1e-6 absolute = 1e-6 relative density
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-9, atol=1e-6)
    from pyabc_amd import gpu
    chol = tr._dev_chol
    th, lp, anc, att = tr.propose_device(5000, seed=77, generation=3, idx0=1000)
    th_o, _, anc_o, _ = osamp.propose_local(X, w, chol.cpu().numpy(), 77, 3, 1000, 5000)
    np.testing.assert_array_equal(anc.cpu().numpy(), anc_o)
    np.testing.assert_allclose(th.cpu().numpy(), th_o, rtol=1e-12, atol=1e-12)


def test_local_transition_wide_generations():
    """ABCSMC with LocalTransition at d = 20 through the batched sampler
    (fused rounds with per-particle factors): every generation's weights
    equal the oracle's prior / LocalTransition density of the previous
    population to 1e-6 relative (north_star's bar: 1e-5)."""
    import pyabc_amd as pa
    d = 20
    names = [f"p{q:02d}" for q in range(d)]
    keys = [f"y{q:02d}" for q in range(d)]
    model = pa.LinearGaussianModel(names, keys, src=list(range(d)), sigma=[0.5] * d)
    prior = pa.Distribution(**{n: pa.RV("norm", 0, 1) for n in names})
    abc = pa.ABCSMC(model, prior, pa.PNormDistance(p=2), population_size=1500,
                    transitions=pa.LocalTransition(k=50, k_fraction=None),
                    sampler=pa.BatchedGPUSampler(seed=3),
                    eps=pa.QuantileEpsilon(alpha=0.5))
    abc.new("sqlite://", {k: 0.5 for k in keys})
    h = abc.run(max_nr_populations=3)
    assert h.max_t == 2
    for t in range(1, h.max_t + 1):
        dfp, wp = h.get_distribution(0, t - 1)
        df, w = h.get_distribution(0, t)
        Xp, x = dfp[names].to_numpy(), df[names].to_numpy()
        fit = oracle.local_fit(Xp, wp, k=50, k_fraction=None)
        lw = stats.norm.logpdf(x).sum(1) - np.log(oracle.local_pdf(x, Xp, fit))
        ref = np.exp(lw - lw.max())
        ref /= ref.sum()
        np.testing.assert_allclose(w, ref, rtol=1e-6, atol=0)


def test_discrete_prior_per_candidate_loop():
    """A poisson prior has no batched form (its pmf vanishes between the
    integers, where the reference re-draws, smc.py:649-662): the generation
    runs the per-candidate loop with DiscreteRandomWalkTransition, so every
    particle is an integer with positive prior mass and positive weight, and
    allow_per_candidate=False turns the fallback into a TypeError."""
    import pyabc_amd as pa
    np.random.seed(21)
    prior = pa.Distribution(k=pa.RV("poisson", 3))
    assert prior.device_spec() is None
    assert pa.Distribution(k=pa.RV("rv_discrete", values=([0, 1], [.5, .5]))) \
        .device_spec() is None

    def model(p):
        return {"y": p["k"] + 0.5 * np.random.randn()}
    sampler = pa.BatchedGPUSampler()
    abc = pa.ABCSMC(model, prior, pa.PNormDistance(), population_size=200,
                    transitions=pa.DiscreteRandomWalkTransition(n_steps=2),
                    sampler=sampler)
    abc.new("sqlite://", {"y": 4.0})
    h = abc.run(max_nr_populations=3)
    assert h.max_t == 2
    assert sampler.last_stats.get("per_candidate")
    for t in range(h.max_t + 1):
        df, w = h.get_distribution(0, t)
        k = df["k"].to_numpy()
        assert np.array_equal(k, np.rint(k)) and (k >= 0).all()
        assert (w > 0).all() and abs(w.sum() - 1) < 1e-12
    strict = pa.BatchedGPUSampler(allow_per_candidate=False)
    abc2 = pa.ABCSMC(model, prior, pa.PNormDistance(), population_size=20,
                     transitions=pa.DiscreteRandomWalkTransition(), sampler=strict)
    abc2.new("sqlite://", {"y": 4.0})
    with pytest.raises(TypeError, match="allow_per_candidate"):
        abc2.run(max_nr_populations=1)


def test_sampler_reused_across_runs():
    """One BatchedGPUSampler (fixed seed) drives two ABCSMC runs in a row; the
    staged path's cached proposal round must belong to the current run: the
    second run equals the same run on a fresh sampler, bit for bit."""
    import pyabc_amd as pa
    names, keys = ["a", "b"], ["y0", "y1"]

    def sim(theta, seed, gen, idx0):
        g = torch.Generator(device=theta.device)
        g.manual_seed((seed * 1000003 + gen * 7919 + idx0) % (2 ** 63))
        return theta + 0.5 * torch.randn(theta.shape, generator=g,
                                          dtype=theta.dtype, device=theta.device)

    def run(sampler, scale):
        prior = pa.Distribution(a=pa.RV("norm", 0, scale), b=pa.RV("norm", 0, scale))
        abc = pa.ABCSMC(pa.VectorizedModel(sim, keys), prior, pa.PNormDistance(p=2),
                        population_size=2000, sampler=sampler,
                        eps=pa.QuantileEpsilon(alpha=0.5))
        abc.new("sqlite://", {"y0": 1.0, "y1": 0.5})
        h = abc.run(max_nr_populations=3)
        return [h.get_distribution(0, t) for t in range(h.max_t + 1)]
    shared = pa.BatchedGPUSampler(seed=9)
    run(shared, 1.0)
    second = run(shared, 3.0)
    fresh = run(pa.BatchedGPUSampler(seed=9), 3.0)
    for (df1, w1), (df2, w2) in zip(second, fresh):
        np.testing.assert_array_equal(df1[names].to_numpy(), df2[names].to_numpy())
        np.testing.assert_array_equal(w1, w2)


def test_user_model_accept_tail_equals_staged():
    """A user VectorizedModel's rounds decide acceptance in the accept tail
    (abc_pnorm_accept); a PNormDistance subclass without the fused form
    takes the staged distance + compaction instead.  Both runs give the same
    populations, weights, epsilons and evaluation counts bit for bit."""
    import pyabc_amd as pa
    names, keys = [f"p{k}" for k in range(4)], [f"y{k}" for k in range(4)]

    class Staged(pa.PNormDistance):
        def weight_vector(self, t, k):          # same values, no fused form
            return super().weight_vector(t, k)

    def sim(theta, seed, gen, idx0):
        g = torch.Generator(device=theta.device)
        g.manual_seed((seed * 1000003 + gen * 7919 + idx0) % (2 ** 63))
        return theta + 0.5 * torch.randn(theta.shape, generator=g, dtype=theta.dtype,
                                          device=theta.device)

    def run(dist):
        prior = pa.Distribution(**{n: pa.RV("norm", 0, 1) for n in names})
        sampler = pa.BatchedGPUSampler(seed=17)
        abc = pa.ABCSMC(pa.VectorizedModel(sim, keys), prior, dist, population_size=3000,
                        sampler=sampler, eps=pa.QuantileEpsilon(alpha=0.5))
        abc.new("sqlite://", {k: 0.7 for k in keys})
        h = abc.run(max_nr_populations=5)
        pops = h.get_all_populations()
        return [h.get_distribution(0, t) for t in range(h.max_t + 1)], pops
    a, pa_ = run(pa.PNormDistance(p=2))
    b, pb_ = run(Staged(p=2))
    assert len(a) == len(b) == 5
    for (df1, w1), (df2, w2) in zip(a, b):
        np.testing.assert_array_equal(df1[names].to_numpy(), df2[names].to_numpy())
        np.testing.assert_array_equal(w1, w2)
    np.testing.assert_array_equal(pa_["epsilon"].to_numpy(), pb_["epsilon"].to_numpy())
    np.testing.assert_array_equal(pa_["samples"].to_numpy(), pb_["samples"].to_numpy())


@pytest.mark.parametrize("accept_tail", [True, False])
def test_user_model_float32_rows(accept_tail):
    """A user VectorizedModel that returns float32 rows: the staged loop
    takes them as their float64 cast in every branch (calibration, accept
    tail, distance + compaction), so the run equals, bit for bit, the run of
    a model returning that cast itself, and its statistics are float64."""
    import pyabc_amd as pa
    names, keys = ["a", "b", "c"], ["y0", "y1", "y2"]

    def sim(dtype):
        def run(theta, seed, gen, idx0):
            g = torch.Generator(device=theta.device)
            g.manual_seed((seed * 1000003 + gen * 7919 + idx0) % (2 ** 63))
            x = theta + 0.5 * torch.randn(theta.shape, generator=g, dtype=theta.dtype,
                                          device=theta.device)
            return x.to(torch.float32).to(dtype)
        return run

    def run(dtype):
        prior = pa.Distribution(**{n: pa.RV("norm", 0, 1) for n in names})
        sampler = pa.BatchedGPUSampler(seed=13, accept_tail=accept_tail)
        abc = pa.ABCSMC(pa.VectorizedModel(sim(dtype), keys), prior, pa.PNormDistance(p=2),
                        population_size=1000, sampler=sampler,
                        eps=pa.QuantileEpsilon(alpha=0.5))
        abc.new("sqlite://", {k: 0.7 for k in keys})
        h = abc.run(max_nr_populations=3)
        cols = h.get_population_device(h.max_t)
        assert cols.sum_stats.dtype == torch.float64
        return ([h.get_distribution(0, t) for t in range(h.max_t + 1)],
                h.get_all_populations(), cols.sum_stats.cpu().numpy())
    a, pa_, xa = run(torch.float32)
    b, pb_, xb = run(torch.float64)
    assert len(a) == len(b) == 3
    for (df1, w1), (df2, w2) in zip(a, b):
        np.testing.assert_array_equal(df1[names].to_numpy(), df2[names].to_numpy())
        np.testing.assert_array_equal(w1, w2)
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(xa, xa.astype(np.float32).astype(np.float64))
    np.testing.assert_array_equal(pa_["epsilon"].to_numpy(), pb_["epsilon"].to_numpy())
    np.testing.assert_array_equal(pa_["samples"].to_numpy(), pb_["samples"].to_numpy())


def test_local_transition_d80_generations():
    """ABCSMC with LocalTransition at d = 80 (> 64: staged rounds with the
    wide propose kernel, the BIG fit and density): every generation's
    weights equal the oracle's prior / LocalTransition density of the
    previous population, row by row within a first-order rounding bound of
    the inverses (the 80-D covariances of 100 neighbours have condition
    numbers up to ~1e10 and beyond).  A backward-stable inverse is the exact
    inverse of A_j + E_j with |E_j| <= c_n u |A_j| componentwise (u = 2^-53,
    c_n = d for an LU with small growth), so to first order the quadratic
    form q_ij = d^T inv_j d moves by |v^T E_j v| <= c_n u |v|^T |A_j| |v|
    (v = inv_j d_ij) and log det_j by |tr(inv_j E_j)| <= c_n u
    tr(|inv_j| |A_j|); both the device's LU and LAPACK's are within that
    of the exact values, hence of each other within twice it.  A
    candidate's log density moves by the responsibility-weighted sum of the
    pair terms (r_ij = share of pair j in its density), its normalised log
    weight by that minus the weighted mean: |dlog w_i| <= b_i + sum_k w_k b_k,
    b_i = sum_j r_ij 2 c_n u (|v|^T |A_j| |v| + tr(|inv_j| |A_j|)) / 2.
    Asserted per row; the worst row's error and bound are printed."""
    import pyabc_amd as pa
    d = 80
    names = [f"p{q:02d}" for q in range(d)]
    keys = [f"y{q:02d}" for q in range(d)]
    model = pa.LinearGaussianModel(names, keys, src=list(range(d)), sigma=[0.5] * d)
    prior = pa.Distribution(**{n: pa.RV("norm", 0, 1) for n in names})
    abc = pa.ABCSMC(model, prior, pa.PNormDistance(p=2), population_size=600,
                    transitions=pa.LocalTransition(k=100, k_fraction=None),
                    sampler=pa.BatchedGPUSampler(seed=13),
                    eps=pa.QuantileEpsilon(alpha=0.5))
    abc.new("sqlite://", {k: 0.3 for k in keys})
    h = abc.run(max_nr_populations=3)
    assert h.max_t == 2
    for t in range(1, h.max_t + 1):
        dfp, wp = h.get_distribution(0, t - 1)
        df, w = h.get_distribution(0, t)
        Xp, x = dfp[names].to_numpy(), df[names].to_numpy()
        fit = oracle.local_fit(Xp, wp, k=100, k_fraction=None)
        lw = stats.norm.logpdf(x).sum(1) - np.log(oracle.local_pdf(x, Xp, fit))
        ref = lw - lw.max()
        ref -= np.log(np.exp(ref).sum())
        bound = _local_weight_bound(x, Xp, fit, np.exp(ref))
        got = np.log(w)
        err = np.abs(got - ref)
        i = int(np.argmax(err))
        print(f"t={t}: max |dlog w| {err[i]:.3e} (row {i}, its bound {bound[i]:.3e}), "
              f"median bound {np.median(bound):.3e}, max ratio {np.max(err / bound):.3e}")
        assert (err <= bound).all(), np.max(err / bound)


def _local_weight_bound(x, Xp, fit, wn):
    """Per-row first-order bound on |dlog w_i| (test_local_transition_d80_generations)."""
    n, d = Xp.shape
    cu = 2.0 * d * 2.0 ** -53
    covs, inv, w = fit["covs"], fit["inv_covs"], fit["w"]
    absA = np.abs(covs)
    tr = np.einsum("jab,jba->j", np.abs(inv), absA)
    b = np.empty(len(x))
    for i in range(len(x)):
        dl = Xp - x[i]
        v = np.einsum("jab,jb->ja", inv, dl)
        q = np.einsum("ja,ja->j", dl, v)
        vav = np.einsum("ja,jab,jb->j", np.abs(v), absA, np.abs(v))
        lt = np.log(w) - 0.5 * q - np.log(fit["normalization"])
        r = np.exp(lt - lt.max())
        r /= r.sum()
        b[i] = np.sum(r * cu * 0.5 * (vav + tr))
    return b + np.sum(wn * b)


@pytest.mark.parametrize("d", [3, 20, 80])
def test_local_fit_degenerate_weights(d):
    """Neighbourhoods where the reference's np.cov(aweights) divides by
    1 - sum a^2 == 0 (one neighbour carries all the weight) or by a zero
    weight sum (tests/golden/local_degenerate.npz, made by importing pyABC,
    local_transition.py:112-139): the device covariances are non-finite for
    exactly the particles whose reference covariances are, the determinant
    loop ends on the NaN determinant as "while det <= 0" does (it used to
    spin to its 10^6-iteration cap), and every finite covariance equals the
    reference's to 1e-9 relative, its determinant to 1e-7.  d = 3 runs the
    register kernels, 20 the runtime-d LDS kernel, 80 the workspace one."""
    import pyabc_amd as pa
    g = np.load(os.path.join(GOLDEN, "local_degenerate.npz"))
    X, w, k = g[f"X{d}"], g[f"w{d}"], int(g[f"k{d}"])
    cols = [f"p{q:02d}" for q in range(d)]
    tr = pa.LocalTransition(k=k, k_fraction=None)
    tr.fit(pd.DataFrame(X, columns=cols), w.copy())
    ref, dets = g[f"covs{d}"], g[f"dets{d}"]
    fin = np.isfinite(ref).all(axis=(1, 2))
    got = tr.covs
    np.testing.assert_array_equal(np.isfinite(got).all(axis=(1, 2)), fin)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(tr.determinants[fin], dets[fin], rtol=1e-7)
