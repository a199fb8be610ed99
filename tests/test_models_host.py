"""Model selection, host side (no GPU): the package's model-jump pmf, model
factor and weight normalisation against values recorded from the reference
(tests/golden/models.npz, make_golden_models.py); the numpy replay's proposal
has the reference's whole-attempt re-draw; GenerationSpec names every case it
leaves to the per-candidate loop."""
import os

import numpy as np
import pytest
from scipy import stats

import models_ref as mref
from conftest import GOLDEN

STAYS = {"none": None, "0.7": 0.7, "1.0": 1.0}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "models.npz"))


@pytest.mark.parametrize("tag", sorted(STAYS))
@pytest.mark.parametrize("M", [1, 2, 5])
def test_perturbation_kernel_pmf(gold, M, tag):
    import pyabc_amd as pa
    k = pa.ModelPerturbationKernel(M, probability_to_stay=STAYS[tag])
    got = np.array([[k.pmf(n, m) for m in range(M)] for n in range(M + 1)])
    want = gold[f"pmf_M{M}_stay{tag}"]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
    np.testing.assert_allclose(mref.kernel_matrix(M, STAYS[tag]), want[:M], rtol=0,
                               atol=1e-15)


@pytest.mark.parametrize("tag", sorted(STAYS))
def test_model_factor(gold, tag):
    import pyabc_amd as pa
    from pyabc_amd.smc import model_proposal_masses
    p_prev = {m: float(p) for m, p in enumerate(gold["P_PREV"])}
    prior = np.full(3, 1.0 / 3)
    k = pa.ModelPerturbationKernel(3, probability_to_stay=STAYS[tag])
    q, factor = model_proposal_masses(p_prev, k, prior)
    want = gold[f"factor_stay{tag}"]
    np.testing.assert_allclose(factor, want, rtol=0, atol=1e-15)
    # the proposal's model law: the same sum, 0 for the dead model
    assert q[1] == 0.0 and q[0] == factor[0] and q[2] == factor[2]
    q_ref, f_ref = mref.model_masses(p_prev, mref.kernel_matrix(3, STAYS[tag]), prior)
    np.testing.assert_allclose(f_ref, want, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(q_ref, q)
    # a model of prior mass 0 is never returned either
    q0, _ = model_proposal_masses(p_prev, k, np.array([0.0, 0.5, 0.5]))
    assert q0[0] == 0.0 and q0[2] == factor[2]


def test_normalisation(gold):
    import pyabc_amd as pa
    parts = [pa.Particle(m=int(m), parameter=pa.Parameter(a=float(i)), weight=float(w),
                         accepted_sum_stats=[{"y": 0.0}], accepted_distances=[float(i)])
             for i, (m, w) in enumerate(zip(gold["NORM_m"], gold["NORM_w"]))]
    pop = pa.Population(parts)
    mp = pop.get_model_probabilities()
    np.testing.assert_allclose([mp[m] for m in range(3)], gold["NORM_p"], rtol=0, atol=1e-15)
    np.testing.assert_allclose([p.weight for p in pop.get_list()], gold["NORM_w_out"],
                               rtol=0, atol=1e-15)
    np.testing.assert_allclose(pop.get_weighted_distances()["w"], gold["NORM_wd"], rtol=0,
                               atol=1e-15)
    p_ref, w_ref = mref.normalize(gold["NORM_m"], gold["NORM_w"])
    np.testing.assert_allclose([p_ref[m] for m in range(3)], gold["NORM_p"], rtol=0,
                               atol=1e-15)
    np.testing.assert_allclose(w_ref, gold["NORM_w_out"], rtol=0, atol=1e-15)


def test_replay_restarts_the_whole_attempt():
    """smc.py:654-656: a theta outside the prior support restarts the attempt,
    the model draw included, so the returned model has marginal ~ q~(m) A_m
    (A_m: model m's in-support mass).  Model 0's proposals (64 ancestors at 0,
    L = 0.3, prior U[0, 1]) are in the support with A_0 = Phi(1 / 0.3) - 1/2;
    model 1's always.  With q~ = (1/2, 1/2) model 0's share of the returned
    candidates is A_0 / (1 + A_0) ~ 0.3331; a re-draw of theta alone in a
    fixed model would return it half the time."""
    B = 200_000
    models = [
        dict(kinds=["uniform"], params=[[0.0, 1.0, 0, 0]], X=np.zeros((64, 1)),
             cdf=np.cumsum(np.full(64, 1.0 / 64)), L=np.array([[0.3]])),
        dict(kinds=["norm", "norm"], params=[[0.0, 1.0, 0, 0]] * 2, X=np.zeros((8, 2)),
             cdf=np.cumsum(np.full(8, 0.125)), L=0.5 * np.eye(2)),
    ]
    model, theta, anc, att, changed = mref.propose(models, [0.5, 1.0], 41, 3, 0, B)
    assert (att <= 1000).all() and changed > 1000
    A0 = stats.norm.cdf(1 / 0.3) - 0.5
    p = A0 / (1 + A0)
    share = np.mean(model == 0)
    print("share of model 0", share, "expected", p)
    assert abs(share - p) <= 5 * np.sqrt(p * (1 - p) / B)
    assert abs(0.5 - p) > 50 * np.sqrt(p * (1 - p) / B)    # the wrong law is far
    th0 = theta[model == 0]
    assert np.isnan(th0[:, 1]).all() and (0 <= th0[:, 0]).all() and (th0[:, 0] <= 1).all()
    assert (anc[model == 0] < 64).all() and (anc[model == 1] < 8).all()


# ---- GenerationSpec.why_not --------------------------------------------------

class _History:
    def __init__(self, probs):
        self.probs = probs

    def model_probabilities_dict(self, t=None):
        return dict(self.probs)


def _abc(M=2, **kw):
    import pyabc_amd as pa
    keys = ["y0", "y1"]
    models = [pa.LinearGaussianModel(["a"], keys, [0, 0], name=f"m{m}") for m in range(M)]
    priors = [pa.Distribution(a=pa.RV("norm", 0, 1)) for _ in range(M)]
    abc = pa.ABCSMC(models, priors, kw.pop("distance", pa.PNormDistance(p=2)),
                    population_size=kw.pop("population_size", 100),
                    sampler=pa.BatchedGPUSampler(), **kw)
    abc.x_0 = {"y0": 0.0, "y1": 0.0}
    abc.history = _History({m: 1.0 / M for m in range(M)})
    return abc


def test_why_not_names_each_excluded_case(monkeypatch):
    import pyabc_amd as pa
    from pyabc_amd.sampler import distributed as dd

    abc = _abc(17)
    spec = pa.GenerationSpec(abc, 0)
    assert not spec.batched_capable and "more than 16 models" in spec.why_not

    abc = _abc(2, transitions=[pa.LocalTransition(), pa.LocalTransition()])
    spec = pa.GenerationSpec(abc, 1)
    assert not spec.batched_capable
    assert "transition of model 0 is not a fitted MultivariateNormalTransition" \
        in spec.why_not

    abc = _abc(2, distance=pa.IndependentNormalKernel(var=[1.0, 1.0]),
               eps=pa.Temperature(), acceptor=pa.StochasticAcceptor())
    spec = pa.GenerationSpec(abc, -1, all_accepted=True)
    assert not spec.batched_capable
    assert "StochasticAcceptor with several models" in spec.why_not

    abc = _abc(2)
    monkeypatch.setattr(dd, "world", lambda: (0, 2))
    spec = pa.GenerationSpec(abc, 0)
    assert not spec.batched_capable and "several ranks" in spec.why_not
    monkeypatch.undo()

    abc = _abc(2, population_size=pa.ConstantPopulationSize(100, nr_samples_per_parameter=2))
    assert "nr_samples_per_parameter != 1" in pa.GenerationSpec(abc, 0).why_not

    abc = _abc(2, summary_statistics=lambda x: x)
    assert "custom summary_statistics" in pa.GenerationSpec(abc, 0).why_not

    # scalar models keep the per-candidate loop, as before
    abc = pa.ABCSMC([lambda p: {"y0": 0.0}, lambda p: {"y0": 1.0}],
                    [pa.Distribution(a=pa.RV("norm", 0, 1))] * 2,
                    sampler=pa.BatchedGPUSampler())
    abc.x_0 = {"y0": 0.0}
    abc.history = _History({0: 0.5, 1: 0.5})
    spec = pa.GenerationSpec(abc, 0)
    assert not spec.batched_capable and "model 0 is not a VectorizedModel" in spec.why_not
    assert spec.models is None

    # one model goes exactly where it went
    one = pa.ABCSMC(lambda p: {"y0": 0.0}, pa.Distribution(a=pa.RV("norm", 0, 1)),
                    sampler=pa.BatchedGPUSampler())
    one.x_0 = {"y0": 0.0}
    spec = pa.GenerationSpec(one, 0)
    assert spec.models is None and spec.why_not == "model is not a VectorizedModel"


# ---- the multi-model candidate source on the staged loop (CPU doubles) --------

_SEED, _S, _BATCH, _N_REPLAY = 4242, 3, 300, 1800
_MODELS = [dict(kinds=["uniform"], params=[[0.0, 1.0, 0, 0]]),
           dict(kinds=["norm", "norm"], params=[[0.0, 1.0, 0, 0]] * 2)]
_SRC = np.array([[0, 0, 0], [0, 1, 0]])
_A = np.array([[1.0, -1.0, 0.5], [1.0, 1.0, -1.0]])
_SIGMA = np.full((2, _S), 0.5)
_EPS = 1.0


def _pnorm_np(x, x0, wf, p):
    return (np.abs(wf * (x - x0)) ** p).sum(1) ** (1.0 / p)


@pytest.fixture(scope="module")
def models_replay():
    """The first _N_REPLAY candidates of generation 0 (candidates are keyed by
    their global index, so rounds of any size see these rows)."""
    model, theta, anc, att, _ = mref.propose(_MODELS, [0.5, 1.0], _SEED, 0, 0, _N_REPLAY,
                                             10000)
    x = mref.simulate(theta, model, _SRC, _A, _SIGMA, _SEED, 0, 0)
    d = _pnorm_np(x, np.zeros(_S), np.ones(_S), 2.0)
    return dict(model=model, theta=theta, x=x, d=d, acc=np.nonzero(d <= _EPS)[0])


class _TableModel:
    def __init__(self, m):
        self.m = m

    def fused_simulator(self, dev):
        import torch
        return (torch.tensor(_SRC[self.m], dtype=torch.int32),
                torch.tensor(_A[self.m]), torch.tensor(_SIGMA[self.m]))


class _ModelsSpec:
    """What the staged loop reads of a GenerationSpec over two models at
    t = 0 (no transitions: the weights are ones)."""
    batched_capable = True

    def __init__(self):
        import torch
        import pyabc_amd as pa
        self.t = 0
        self.sum_stat_keys = [f"y{k}" for k in range(_S)]
        self.distance = pa.PNormDistance(p=2)
        self.x0vec = torch.zeros(_S, dtype=torch.float64)
        self.eps = _EPS
        self.weight_scale = 1.0
        self.models = dict(
            M=2, d=[1, 2], param_names=[["a"], ["a", "b"]],
            prior_kind=[torch.zeros(d, dtype=torch.int32) for d in (1, 2)],
            prior_params=[torch.zeros(4 * d, dtype=torch.float64) for d in (1, 2)],
            transitions=[None, None], vmodels=[_TableModel(0), _TableModel(1)],
            model_cdf=np.array([0.5, 1.0]), masses=np.array([0.5, 0.5]),
            log_scale=np.zeros(2))


def _install_models_doubles(monkeypatch):
    """The device calls of a multi-model staged round as the numpy replay
    (models_ref) and index arithmetic, on host tensors."""
    import torch
    from pyabc_amd.sampler import batched
    g = batched.gpu
    t = torch.from_numpy

    class ModelSet:
        def __init__(self, descs, model_cdf, seed, generation, max_attempts):
            self.args = (model_cdf, seed, generation)
            self.max_attempts = max_attempts

        def propose(self, idx0, B):
            model, theta, anc, att, _ = mref.propose(_MODELS, *self.args, idx0, B,
                                                     self.max_attempts)
            return t(model).to(torch.int32), t(theta), t(anc), t(att).to(torch.int32)

    def simulate(theta, model, src, a, sigma, seed, generation, idx0):
        return t(mref.simulate(theta.numpy(), model.numpy(), src.numpy(), a.numpy(),
                               sigma.numpy(), seed, generation, idx0))

    def partition(model, M):
        perm, counts = mref.partition(model.numpy(), M)
        return t(perm), t(counts)

    def pnorm(x, x0, wf, pv, out=None):
        return t(_pnorm_np(x.numpy(), x0.numpy(), wf.numpy(), pv))

    def pnorm_accept(x, x0, wf, pv, eps, cap, att=None, max_attempts=0):
        d = _pnorm_np(x.numpy(), x0.numpy(), wf.numpy(), pv)
        acc = np.nonzero((d <= eps) & (att.numpy() <= max_attempts))[0]
        idx = torch.zeros(max(int(cap), 1), dtype=torch.int64)
        k = min(int(cap), len(acc))
        idx[:k] = t(acc[:k])
        return idx, torch.tensor([len(acc)])

    def accept_compact(d, eps):
        idx = torch.nonzero(d <= eps).flatten().to(torch.int64)
        return idx, torch.tensor([idx.numel()])

    def mask_gave_up(dist, att, max_attempts, value=float("nan")):
        dist[att > max_attempts] = value
        return dist

    for name, fn in dict(
            ModelSet=ModelSet, models_simulate_linear_gaussian=simulate,
            models_partition=partition, pnorm=pnorm, pnorm_accept=pnorm_accept,
            accept_compact=accept_compact, mask_gave_up=mask_gave_up,
            require_device=lambda: torch.device("cpu"),
            gather_rows=lambda x, idx, n=None: x.index_select(0, idx),
            gather_rows_batch=lambda arrays, idx, n=None: [a.index_select(0, idx)
                                                           for a in arrays]).items():
        monkeypatch.setattr(g, name, fn)


@pytest.mark.parametrize("record", [False, True])
@pytest.mark.parametrize("accept_tail", [True, False])
def test_models_source_on_the_staged_loop(monkeypatch, models_replay, accept_tail, record):
    """BatchedGPUSampler's staged loop with its multi-model candidate source
    (M = 2, d = (1, 2), S = 3, t = 0) on one rank, the device calls replaced
    by the replay: n = 200 at 300 candidates per round takes 3 rounds and
    cuts the last one in the middle.  The kept rows are the replay's first
    200 accepted, split by model in candidate order; the evaluations end at
    the 200th accepted; the recorded matrix is every row up to it; the accept
    tail and the distance + compaction branch give the same sample."""
    from pyabc_amd.sampler import BatchedGPUSampler
    n, rp = 200, models_replay
    acc = rp["acc"]
    assert 0.15 <= len(acc) / _N_REPLAY <= 0.40
    _install_models_doubles(monkeypatch)
    s = BatchedGPUSampler(batch_size=_BATCH, seed=_SEED, accept_tail=accept_tail)
    s.sample_factory.record_rejected = record
    sample = s.sample_until_n_accepted(n, _ModelsSpec())
    assert sample.ok and sample.n_accepted == n
    assert s.last_stats["rounds"] >= 2
    assert s.nr_evaluations_ == acc[n - 1] + 1
    assert s.nr_evaluations_ % _BATCH not in (0, 1, _BATCH - 1)    # cut mid-round
    first = acc[:n]
    per_model = {}
    for m, d in enumerate((1, 2)):
        rows = first[rp["model"][first] == m]
        per_model[m] = len(rows)
        c = sample._mcols[m]
        np.testing.assert_array_equal(c.theta.numpy(), rp["theta"][rows, :d])
        np.testing.assert_array_equal(c.sum_stats.numpy(), rp["x"][rows])
        np.testing.assert_array_equal(c.distances.numpy(), rp["d"][rows])
        np.testing.assert_array_equal(c.weights.numpy(), np.ones(len(rows)))
        assert c.param_names == [["a"], ["a", "b"]][m] and c.m == m
    assert min(per_model.values()) > 0
    assert s.last_stats["accepted_per_model"] == per_model
    assert s.last_stats["models"] == 2 and s.last_stats["accepted"] == n
    assert s.last_stats["evaluations"] == s.nr_evaluations_
    assert not s.last_stats["records_truncated"]
    want = (rp["x"][:s.nr_evaluations_] if record else
            np.concatenate([rp["x"][first[rp["model"][first] == m]] for m in (0, 1)]))
    np.testing.assert_array_equal(sample._recorded.numpy(), want)
