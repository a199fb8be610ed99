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
