"""Model selection on the device: the multi-model proposal, simulator and
partition kernels against the numpy replay (tests/models_ref.py), one sampler
round against the replayed rounds, and ABCSMC runs over two models against
the exact uniform-kernel ABC posterior.  Integer work (models, ancestors,
attempts, the partition) is exact; theta and the statistics meet the existing
replay tests' bars; weights carry the density kernel's 2e-6 twice."""
import logging

import numpy as np
import pytest
from scipy import integrate, stats

import models_ref as mref
import oracle
import oracle.sampler as osamp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    from pyabc_amd import gpu
    return gpu.require_device()


def T(a, dtype=None):
    from pyabc_amd import gpu
    return gpu.as_dev(a, dtype=dtype)


def dev_models(models):
    """Device descriptors (gpu.ModelSet) of replay models."""
    out = []
    for m in models:
        d = dict(d=len(m["kinds"]),
                 prior_kind=T([osamp.KIND[k] for k in m["kinds"]], dtype=torch.int32),
                 prior_params=T(np.asarray(m["params"], dtype=np.float64).ravel()))
        if m.get("X") is not None:
            d.update(X=T(m["X"]), cdf=T(m["cdf"]), L=T(m["L"]))
        out.append(d)
    return out


def population(rng, N, d, loc=0.0):
    X = loc + rng.standard_normal((N, d))
    w = rng.uniform(0.5, 1.5, size=N)
    w /= w.sum()
    A = rng.standard_normal((d, d))
    L = np.linalg.cholesky(A @ A.T / d + np.eye(d)) * 0.4
    return dict(X=X, w=w, cdf=np.cumsum(w), L=L)


# ---- 1. one model: abc_propose's rows bit for bit -----------------------------

def test_one_model_equals_single_model_proposal(dev):
    from pyabc_amd import gpu
    rng = np.random.default_rng(6)              # test_propose_replay's inputs
    N, d = 1000, 3
    X = rng.standard_normal((N, d))
    w = rng.uniform(size=N)
    w /= w.sum()
    L = np.linalg.cholesky(np.array([[1, .3, 0], [.3, 1, .2], [0, .2, .5]])) * .4
    kinds = ["uniform", "norm", "expon"]
    params = np.array([[-1.0, 2.0, 0, 0], [0.0, 1.0, 0, 0], [-0.5, 1.0, 0, 0]])
    kd = T([osamp.KIND[k] for k in kinds], dtype=torch.int32)
    pd_ = T(params.ravel())
    cdf = gpu.inclusive_scan(T(w))
    B, idx0 = 5000, 1000
    for prior_mode in (False, True):
        desc = dict(d=d, prior_kind=kd, prior_params=pd_)
        if prior_mode:
            th, _, anc, att = gpu.propose(None, None, None, kd, pd_, 123, 4, idx0, B, 1000, d)
        else:
            desc.update(X=T(X), cdf=cdf, L=T(L))
            th, _, anc, att = gpu.propose(desc["X"], cdf, desc["L"], kd, pd_, 123, 4, idx0,
                                          B, 1000, d)
        ms = gpu.ModelSet([desc], [1.0], 123, 4, 1000)
        model, th_m, anc_m, att_m = ms.propose(idx0, B)
        assert torch.equal(th_m, th) and torch.equal(att_m, att)
        assert int(model.abs().max()) == 0
        if prior_mode:
            assert int((anc_m != -1).sum()) == 0
        else:
            assert torch.equal(anc_m, anc)
            assert int((att > 1).sum()) > 0          # re-draws happened
        # the guide-table search draws the same ancestors
        if not prior_mode:
            desc["guide"] = gpu.cdf_guide(cdf)
            got = gpu.ModelSet([desc], [1.0], 123, 4, 1000).propose(idx0, B)
            assert torch.equal(got[1], th) and torch.equal(got[2], anc)


# ---- 2. four models against the replay -----------------------------------------

def four_models():
    rng = np.random.default_rng(17)
    dims, Ns = (1, 2, 5, 17), (300, 1, 4097, 64)
    models = []
    for d, N in zip(dims, Ns):
        m = population(rng, N, d)
        m["kinds"] = ["norm"] * d
        m["params"] = np.tile([0.0, 3.0, 0, 0], (d, 1))
        models.append(m)
    # model 0: its box cuts about half of its proposals
    models[0]["kinds"] = ["uniform"]
    models[0]["params"] = np.array([[0.0, 6.0, 0, 0]])
    models[2]["kinds"] = ["norm", "laplace", "uniform", "norm", "expon"]
    models[2]["params"] = np.array([[0.0, 3.0, 0, 0], [0.0, 2.0, 0, 0], [-6.0, 12.0, 0, 0],
                                    [0.5, 2.0, 0, 0], [-5.0, 2.0, 0, 0]])
    return models


def test_four_models_against_replay(dev):
    from pyabc_amd import gpu
    models = four_models()
    q = np.array([0.3, 0.0, 0.5, 0.2])
    B, idx0 = 20000, 2 ** 32 - 100
    ref = mref.propose(models, np.cumsum(q), 77, 5, idx0, B, max_attempts=50)
    assert ref[4] >= 100          # candidates that changed model between attempts
    ms = gpu.ModelSet(dev_models(models), np.cumsum(q), 77, 5, 50)
    model, theta, anc, att = (t.cpu().numpy() for t in ms.propose(idx0, B))
    np.testing.assert_array_equal(model, ref[0])
    np.testing.assert_array_equal(anc, ref[2])
    np.testing.assert_array_equal(att, ref[3])
    assert theta.shape == (B, 17)
    np.testing.assert_array_equal(np.isnan(theta), np.isnan(ref[1]))
    np.testing.assert_allclose(theta, ref[1], rtol=1e-12, atol=1e-13)
    for m, d in enumerate((1, 2, 5, 17)):
        rows = theta[model == m]
        assert np.isnan(rows[:, d:]).all() and not np.isnan(rows[:, :d]).any()
    assert not (model == 1).any()                    # the dead model
    share = np.mean(att[model == 0] == 1)
    assert (att > 1).sum() > 1000 and (att <= 50).all(), share


def test_prior_draw_against_replay(dev):
    from pyabc_amd import gpu
    models = [
        dict(kinds=["uniform"], params=[[0.7, 2.0, 0, 0]]),
        dict(kinds=["norm", "lognorm"], params=[[0.5, 1.0, 0, 0], [0.5, 0.0, 1.0, 0]]),
        dict(kinds=["norm", "laplace", "expon", "uniform", "norm"],
             params=[[0, 1, 0, 0], [1, 2, 0, 0], [0.5, 2, 0, 0], [-1, 3, 0, 0], [3, .1, 0, 0]]),
    ]
    cdf = np.cumsum([0.2, 0.5, 0.3])
    B, idx0 = 20000, 2 ** 32 - 100
    ref = mref.propose(models, cdf, 9, 0, idx0, B, max_attempts=10)
    ms = gpu.ModelSet(dev_models(models), cdf, 9, 0, 10)
    model, theta, anc, att = (t.cpu().numpy() for t in ms.propose(idx0, B))
    np.testing.assert_array_equal(model, ref[0])
    np.testing.assert_allclose(theta, ref[1], rtol=1e-12, atol=1e-13)
    assert (att == 1).all() and (anc == -1).all()
    assert set(np.unique(model)) == {0, 1, 2}


# ---- 3. giving up ---------------------------------------------------------------

def test_giving_up(dev):
    from pyabc_amd import gpu
    rng = np.random.default_rng(3)
    m0 = population(rng, 50, 1)
    m0.update(kinds=["uniform"], params=np.array([[100.0, 1.0, 0, 0]]))   # out of reach
    m1 = population(rng, 50, 2)
    m1.update(kinds=["norm"] * 2, params=np.tile([0.0, 1.0, 0, 0], (2, 1)))
    B = 3000
    ms = gpu.ModelSet(dev_models([m0, m1]), [1.0, 1.0], 5, 2, 2)
    model, theta, anc, att = ms.propose(0, B)
    assert int((att != 3).sum()) == 0 and int(model.abs().max()) == 0
    ref = mref.propose([m0, m1], [1.0, 1.0], 5, 2, 0, B, max_attempts=2)
    np.testing.assert_array_equal(anc.cpu().numpy(), ref[2])     # the last attempt's
    np.testing.assert_allclose(theta.cpu().numpy(), ref[1], rtol=1e-12, atol=1e-13)
    # the sampler's accept step rejects every such row, at any threshold
    S = 2
    tab = (T(np.zeros((2, S)), dtype=torch.int32), T(np.ones((2, S))), T(np.ones((2, S))))
    x = gpu.models_simulate_linear_gaussian(theta, model, *tab, 5, 2, 0)
    one = T(np.ones(S))
    idx, cnt = gpu.pnorm_accept(x, T(np.zeros(S)), one, 2.0, np.inf, B, att=att,
                                max_attempts=2)
    assert int(cnt.item()) == 0
    dist = gpu.mask_gave_up(gpu.pnorm(x, T(np.zeros(S)), one, 2.0), att, 2)
    assert int(gpu.accept_compact(dist, np.inf)[1].item()) == 0


# ---- 4. simulator -----------------------------------------------------------------

def test_simulator_against_replay(dev):
    from pyabc_amd import gpu
    rng = np.random.default_rng(8)
    B, S, dims = 4097, 7, (1, 3, 5)
    model = rng.integers(0, 3, size=B)
    theta = np.full((B, 5), np.nan)
    for m, d in enumerate(dims):
        theta[model == m, :d] = rng.standard_normal(((model == m).sum(), d))
    src = np.stack([np.arange(S) % d for d in dims])
    src[2] = src[2][::-1]
    a = rng.uniform(0.5, 2, (3, S))
    sig = 10 ** rng.uniform(-2, 2, (3, S))
    x = gpu.models_simulate_linear_gaussian(
        T(theta), T(model, dtype=torch.int32), T(src, dtype=torch.int32), T(a), T(sig),
        55, 3, 2 ** 32 - 7).cpu().numpy()
    ref = mref.simulate(theta, model, src, a, sig, 55, 3, 2 ** 32 - 7)
    np.testing.assert_allclose(x, ref, rtol=1e-12, atol=1e-12)
    # one model: the single-model kernel's bits
    th1 = T(rng.standard_normal((B, 3)))
    one = gpu.models_simulate_linear_gaussian(
        th1, torch.zeros(B, dtype=torch.int32, device=dev), T(src[1:2], dtype=torch.int32),
        T(a[1:2]), T(sig[1:2]), 55, 3, 10)
    single = gpu.simulate_linear_gaussian(th1, T(src[1], dtype=torch.int32), T(a[1]),
                                          T(sig[1]), 55, 3, 10)
    assert torch.equal(one, single)


# ---- 5. partition -----------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 3, 16])
def test_partition(dev, M):
    from pyabc_amd import gpu
    rng = np.random.default_rng(M)
    for B in (1, 63, 64, 65, 4097, 1_000_003):
        ids = rng.integers(0, M, size=B)
        if M == 16:                         # two empty groups
            ids[ids == 5] = 4
            ids[ids == 15] = 0
        perm, counts = gpu.models_partition(T(ids, dtype=torch.int32), M)
        want_perm, want_counts = mref.partition(ids, M)
        np.testing.assert_array_equal(counts.cpu().numpy(), want_counts)
        np.testing.assert_array_equal(perm.cpu().numpy(), want_perm)
    ids = rng.integers(0, M, size=4097)
    ids[2500] = M
    with pytest.raises(ValueError, match="model id"):
        gpu.models_partition(T(ids, dtype=torch.int32), M)


# ---- 6. one sampler round against the replayed rounds ----------------------------

class _History:
    def __init__(self, probs):
        self.probs = probs

    def model_probabilities_dict(self, t=None):
        return dict(self.probs)


def test_sampler_round_against_replay(dev):
    import pandas as pd
    import pyabc_amd as pa
    rng = np.random.default_rng(12)
    keys = ["y0", "y1", "y2"]
    src = [[0, 0, 0], [0, 1, 0]]
    sig = [[0.5, 0.7, 0.4], [0.3, 0.5, 0.6]]
    names = [["a"], ["b0", "b1"]]
    vm = [pa.LinearGaussianModel(names[m], keys, src[m], sigma=sig[m]) for m in range(2)]
    priors = [pa.Distribution(a=pa.RV("uniform", 0.2, 1.5)),
              pa.Distribution(b0=pa.RV("norm", 0.5, 1.0), b1=pa.RV("norm", 0.0, 2.0))]
    pmf = [0.4, 0.6]
    eps = 0.9
    sampler = pa.BatchedGPUSampler(batch_size=1500, seed=99, allow_per_candidate=False)
    abc = pa.ABCSMC(vm, priors, pa.PNormDistance(p=2), population_size=500,
                    model_prior=pa.RV("rv_discrete", values=([0, 1], pmf)),
                    model_perturbation_kernel=pa.ModelPerturbationKernel(2, 0.8),
                    eps=pa.ListEpsilon([2.0, eps]), sampler=sampler)
    abc.x_0 = {"y0": 0.8, "y1": 0.6, "y2": 0.9}
    p_prev = {0: 0.35, 1: 0.65}
    abc.history = _History(p_prev)
    pops = [population(rng, 300, 1, loc=0.9), population(rng, 257, 2, loc=0.6)]
    for m in range(2):
        abc.transitions[m].fit(pd.DataFrame(pops[m]["X"], columns=names[m]), pops[m]["w"])
    spec = pa.GenerationSpec(abc, 1)
    assert spec.batched_capable, spec.why_not
    sample = sampler.sample_until_n_accepted(500, spec)
    pop = sample.get_accepted_population()

    # the replay, from the very arrays the transitions hold
    trs = abc.transitions
    models = [dict(kinds=["uniform"], params=np.array([[0.2, 1.5, 0, 0]])),
              dict(kinds=["norm", "norm"], params=np.array([[0.5, 1.0, 0, 0],
                                                            [0.0, 2.0, 0, 0]]))]
    for m in range(2):
        models[m].update(X=pops[m]["X"], w=pops[m]["w"],
                         cdf=trs[m]._dev_cdf.cpu().numpy(), L=trs[m]._dev_L.cpu().numpy())
    q, mf = mref.model_masses(p_prev, mref.kernel_matrix(2, 0.8), pmf)
    np.testing.assert_allclose(spec.models["model_cdf"], np.cumsum(q), rtol=1e-15)
    Bt = 6 * 1500
    model, theta, anc, att, _ = mref.propose(models, np.cumsum(q), 99, 1, 0, Bt,
                                             max_attempts=sampler.max_attempts)
    x = mref.simulate(theta, model, np.array(src), np.ones((2, 3)), np.array(sig), 99, 1, 0)
    dist = oracle.pnorm(x, np.array([0.8, 0.6, 0.9]))
    acc = np.nonzero(dist <= eps)[0]
    assert len(acc) >= 500 and (np.abs(dist - eps) > 1e-9).all()
    acc = acc[:500]
    assert sampler.nr_evaluations_ == acc[-1] + 1
    assert sampler.last_stats["models"] == 2
    per = {m: int((model[acc] == m).sum()) for m in range(2)}
    assert sampler.last_stats["accepted_per_model"] == per and min(per.values()) > 20
    w_ref = mref.weights(model[acc], theta[acc], models, mf, pmf, [tr.cov for tr in trs])
    p_ref, wn_ref = mref.normalize(model[acc], w_ref)
    got_p = pop.get_model_probabilities()
    for m in range(2):
        c = pop.model_columns[m]
        rows = acc[model[acc] == m]
        # the kept candidates, in candidate order
        np.testing.assert_allclose(c.sum_stats.cpu().numpy(), x[rows], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(c.theta.cpu().numpy(), theta[rows][:, :len(names[m])],
                                   rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(c.distances.cpu().numpy(), dist[rows], rtol=1e-12)
        np.testing.assert_allclose(c.weights.cpu().numpy(), wn_ref[model[acc] == m],
                                   rtol=4e-6)
        assert abs(got_p[m] - p_ref[m]) <= 4e-6 * p_ref[m]
    wd = pop.get_weighted_distances()
    np.testing.assert_allclose(wd.device_w.sum().item(), 1.0, rtol=1e-12)
    assert len(pop) == 500


# ---- 7. - 9. ABCSMC over two models -----------------------------------------------

KEYS = ["y0", "y1"]
SIGMA = 0.5
PMF = [0.25, 0.75]


def model_pair(user=False):
    import pyabc_amd as pa
    from pyabc_amd import gpu
    A = pa.LinearGaussianModel(["a"], KEYS, [0, 0], sigma=[SIGMA] * 2, name="A")
    B = pa.LinearGaussianModel(["b0", "b1"], KEYS, [0, 1], sigma=[SIGMA] * 2, name="B")
    if user:
        def wrap(mod):
            def run(theta, seed, generation, idx0):
                return gpu.simulate_linear_gaussian(theta, *mod._device_arrays(theta.device),
                                                    seed, generation, idx0)
            return pa.VectorizedModel(run, KEYS, name="user" + mod.name)
        A, B = wrap(A), wrap(B)
    priors = [pa.Distribution(a=pa.RV("uniform", 0.7, 2.0)),
              pa.Distribution(b0=pa.RV("norm", 0.5, 1.0), b1=pa.RV("norm", 0.5, 1.0))]
    return [A, B], priors


def posterior_B(eps, x0):
    """The uniform-kernel ABC posterior probability of model B at threshold
    eps (max norm): evidence_m = P(|x_k - x0_k| <= eps, k = 0, 1 | m)."""
    s = np.sqrt(SIGMA ** 2 + 1.0)
    zb = np.prod([stats.norm.cdf((v + eps - 0.5) / s) - stats.norm.cdf((v - eps - 0.5) / s)
                  for v in x0])

    def f(th):
        return 0.5 * np.prod([stats.norm.cdf((v + eps - th) / SIGMA)
                              - stats.norm.cdf((v - eps - th) / SIGMA) for v in x0])
    za = integrate.quad(f, 0.7, 2.7, epsabs=1e-13, epsrel=1e-11)[0]
    return PMF[1] * zb / (PMF[1] * zb + PMF[0] * za)


def test_model_probabilities_end_to_end(dev):
    """|p_B - exact| <= 5 sqrt(p (1 - p) / ESS_t) at every generation; the
    sampler refuses the per-candidate loop, which two models took before."""
    import pyabc_amd as pa
    eps = [1.2, 0.74, 0.45, 0.27, 0.16]
    x0 = (1.0, 0.6)
    models, priors = model_pair()
    sampler = pa.BatchedGPUSampler(allow_per_candidate=False, seed=20241)
    abc = pa.ABCSMC(models, priors, pa.PNormDistance(p=np.inf), population_size=20000,
                    model_prior=pa.RV("rv_discrete", values=([0, 1], PMF)),
                    model_perturbation_kernel=pa.ModelPerturbationKernel(2, 0.9),
                    eps=pa.ListEpsilon(eps), sampler=sampler)
    abc.new("sqlite://", dict(zip(KEYS, x0)))
    h = abc.run(minimum_epsilon=0.0, max_nr_populations=len(eps))
    assert h.max_t == len(eps) - 1 and sampler.last_stats["models"] == 2
    for t, e in enumerate(eps):
        p = posterior_B(e, x0)
        got = float(h.get_model_probabilities(t).p[1])
        ess = abc.generation_log[t]["ess"]
        bound = 5 * np.sqrt(p * (1 - p) / ess)
        print(f"t={t} eps={e} p_B={got:.5f} exact={p:.5f} bound={bound:.5f} ess={ess:.0f}")
        assert abs(got - p) <= bound, (t, got, p, bound)
        df, w = h.get_distribution(m=1, t=t)
        assert list(df.columns) == ["b0", "b1"] and abs(w.sum() - 1) < 1e-12
        df, w = h.get_distribution(m=0, t=t)
        assert list(df.columns) == ["a"] and abs(w.sum() - 1) < 1e-12


def test_model_death(dev, caplog):
    """x_0 = (6, 6) is out of model A's reach (its statistics have mean <=
    2.7, sigma 0.5) once eps is 1: A dies, and the run goes on, or stops,
    with one model alive."""
    import pyabc_amd as pa
    eps = [3.0, 1.0, 0.6]
    for stop in (False, True):
        models, priors = model_pair()
        sampler = pa.BatchedGPUSampler(allow_per_candidate=False, seed=7)
        abc = pa.ABCSMC(models, priors, pa.PNormDistance(p=np.inf), population_size=500,
                        model_prior=pa.RV("rv_discrete", values=([0, 1], PMF)),
                        model_perturbation_kernel=pa.ModelPerturbationKernel(2, 0.9),
                        eps=pa.ListEpsilon(eps), sampler=sampler,
                        stop_if_only_single_model_alive=stop)
        abc.new("sqlite://", {"y0": 6.0, "y1": 6.0})
        with caplog.at_level(logging.INFO, logger="ABC"):
            caplog.clear()
            h = abc.run(minimum_epsilon=0.0, max_nr_populations=3)
        assert set(h.get_model_probabilities(0).index) == {0, 1}
        mp = h.get_model_probabilities()
        assert list(mp.index) == [1] and abs(float(mp.p[1]) - 1.0) < 1e-12
        assert h.alive_models() == [1]
        df, w = h.get_distribution(m=1)
        assert len(df) == 500 and abs(w.sum() - 1.0) < 1e-12
        assert sampler.last_stats["models"] == 2         # still the new loop
        assert sampler.last_stats["accepted_per_model"] == {1: 500}
        stopped = any("single model alive" in r.getMessage() for r in caplog.records)
        assert stopped == stop and h.max_t == (1 if stop else 2)


def test_user_vectorized_models(dev):
    import pyabc_amd as pa
    models, priors = model_pair(user=True)
    sampler = pa.BatchedGPUSampler(allow_per_candidate=False, seed=31)
    abc = pa.ABCSMC(models, priors, pa.PNormDistance(p=2), population_size=2000,
                    model_prior=pa.RV("rv_discrete", values=([0, 1], PMF)),
                    eps=pa.MedianEpsilon(), sampler=sampler)
    abc.new("sqlite://", {"y0": 1.0, "y1": 0.6})
    h = abc.run(minimum_epsilon=0.0, max_nr_populations=3)
    assert h.max_t == 2 and sampler.last_stats["models"] == 2
    for t in range(3):
        mp = h.get_model_probabilities(t)
        assert abs(float(mp.p.sum()) - 1.0) < 1e-12 and len(mp) == 2
        assert len(h.get_population(t)) == 2000


def test_adaptive_distance_records_rejected(dev):
    """AdaptivePNormDistance asks for the rejected candidates' statistics:
    the multi-model rounds record them as the staged loop does, every
    evaluated candidate up to the n-th accepted, in candidate order."""
    import pyabc_amd as pa
    models, priors = model_pair()
    sampler = pa.BatchedGPUSampler(allow_per_candidate=False, seed=5, batch_size=3000)
    dist = pa.AdaptivePNormDistance(p=2)
    abc = pa.ABCSMC(models, priors, dist, population_size=1000,
                    model_prior=pa.RV("rv_discrete", values=([0, 1], PMF)),
                    eps=pa.MedianEpsilon(), sampler=sampler)
    abc.new("sqlite://", {"y0": 1.0, "y1": 0.6})
    seen = []
    orig = sampler.sample_until_n_accepted

    def spy(n, spec, *a, **k):
        sample = orig(n, spec, *a, **k)
        if not k.get("all_accepted", False):
            seen.append((sample.record_rejected, len(sample.first_m_sum_stats(np.inf)),
                         sampler.nr_evaluations_))
        return sample
    sampler.sample_until_n_accepted = spy
    h = abc.run(minimum_epsilon=0.0, max_nr_populations=3)
    assert h.max_t == 2 and sampler.last_stats["models"] == 2
    assert len(seen) == 3 and all(rec for rec, _, _ in seen)
    for _, rows, n_eval in seen:
        assert rows == n_eval
    # the weights changed between generations (the update saw the records)
    w0, w2 = dist.weights[0], dist.weights[2]
    assert any(abs(w0[k] - w2[k]) > 1e-6 * abs(w0[k]) for k in KEYS)
    mp = h.get_model_probabilities()
    assert abs(float(mp.p.sum()) - 1.0) < 1e-12
