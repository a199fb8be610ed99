"""Host-side API pieces of the drop-in that need no GPU: prior decorators
(random_variables.py:199-325), the discrete random-walk transition
(transition/randomwalk.py), which priors have a batched form, and
ModelPerturbationKernel's argument checks (random_variables.py:455-538)."""
import numpy as np
import pandas as pd
import pytest
from scipy import stats

import pyabc_amd as pa
from pyabc_amd.transition.randomwalk import walk_step_law


def _walk_law_multinomial(s, n, p_l, p_r, p_c):
    """The reference's per-coordinate sum (randomwalk.py:99-118) over
    scipy's multinomial pmf."""
    total = 0.0
    for n_r in range(max(s, 0), n + 1):
        n_l = n_r - s
        total += stats.multinomial.pmf(x=[n_l, n_r, n - n_r - n_l], n=n,
                                       p=[p_l, p_r, p_c])
    return total


@pytest.mark.parametrize("n,probs", [(1, (1 / 3, 1 / 3, 1 / 3)), (2, (.2, .5, .3)),
                                     (4, (.1, .1, .8)), (6, (.45, .45, .1))])
def test_walk_step_law(n, probs):
    law = walk_step_law(n, *probs)
    assert abs(law.sum() - 1) < 1e-14
    for s in range(-n, n + 1):
        assert abs(law[s + n] - _walk_law_multinomial(s, n, *probs)) < 1e-14


def test_random_walk_transition_pdf_rvs():
    rng = np.random.default_rng(4)
    X = pd.DataFrame(rng.integers(-3, 4, (60, 2)).astype(float), columns=["a", "b"])
    w = rng.uniform(size=60)
    tr = pa.DiscreteRandomWalkTransition(n_steps=2, p_l=.25, p_r=.35, p_c=.4)
    tr.fit(X, w)
    x = pd.DataFrame(rng.integers(-5, 6, (25, 2)).astype(float), columns=["a", "b"])
    want = np.array([sum(wj * np.prod([_walk_law_multinomial(int(xi[k] - Xj[k]), 2,
                                                             .25, .35, .4)
                                       for k in range(2)])
                         for Xj, wj in zip(X.values, tr.w)) for xi in x.values])
    np.testing.assert_allclose(tr.pdf(x), want, rtol=1e-12, atol=1e-300)
    assert abs(tr.pdf(x.iloc[3]) - want[3]) < 1e-15
    with pytest.raises(ValueError):
        tr.pdf(pd.DataFrame([[0.5, 1.0]], columns=["a", "b"]))
    np.random.seed(1)
    draws = tr.rvs(4000)
    assert list(draws.columns) == ["a", "b"]
    assert np.array_equal(draws.values, np.rint(draws.values))
    # every draw is within n_steps of some particle and has positive mass
    assert (tr.pdf(draws.iloc[:200]) > 0).all()
    assert tr.rvs_single().shape == (2,)


def test_lower_bound_decorator():
    rv = pa.LowerBoundDecorator(pa.RV("norm", 0, 1), 0.5)
    mass = 1 - stats.norm.cdf(0.5)
    assert rv.pdf(0.4) == 0 and rv.cdf(0.5) == 0
    assert abs(rv.pdf(1.0) - stats.norm.pdf(1.0) / mass) < 1e-15
    assert abs(rv.cdf(1.2) - (stats.norm.cdf(1.2) - stats.norm.cdf(.5)) / mass) < 1e-15
    np.random.seed(0)
    assert all(rv.rvs() > 0.5 for _ in range(200))
    assert repr(rv).startswith("[Lower: X > 0.500000]<RV(name=norm")
    cp = rv.copy()
    assert cp.lower_bound == 0.5 and cp is not rv
    with pytest.raises(Exception, match="measure zero"):
        pa.LowerBoundDecorator(pa.RV("uniform", 0, 1), 1.0)
    pois = pa.LowerBoundDecorator(pa.RV("poisson", 2), 1)
    assert pois.pmf(1) == 0 and abs(pois.pmf(2) - stats.poisson.pmf(2, 2)
                                    / (1 - stats.poisson.cdf(1, 2))) < 1e-15
    assert pa.Distribution(x=rv).device_spec() is None
    assert repr(pa.RVDecorator(pa.RV("norm"))).startswith("[Decorator]")


def test_batched_form_of_priors():
    from pyabc_amd._native import PRIOR_KINDS as K
    assert pa.RV("norm", 1, 2).device_spec() == (K["norm"], [1.0, 2.0, 0.0, 0.0])
    assert pa.RV("t", 3).device_spec()[0] == K["host"]
    for rv in (pa.RV("poisson", 3), pa.RV("binom", 5, .3), pa.RV("randint", 0, 4),
               pa.RV("rv_discrete", values=([0, 2], [.5, .5]))):
        assert rv.device_spec() is None
        assert pa.Distribution(x=rv, y=pa.RV("norm")).device_spec() is None
        assert rv.is_discrete


def _spec_logpdf(kind_name, par, x):
    """The density the device evaluates for (kind, [shape.., loc, scale]):
    scipy's family called with exactly those values, positionally."""
    n = {"norm": 2, "uniform": 2, "expon": 2, "laplace": 2, "lognorm": 3,
         "gamma": 3, "beta": 4}[kind_name]
    return getattr(stats, kind_name).logpdf(x, *par[:n])


# (family, positional / keyword / mixed construction, [shape.., loc, scale])
_FAMILY_FORMS = [
    ("norm", [((1.5, 2.0), {}), ((), dict(loc=1.5, scale=2.0)), ((1.5,), dict(scale=2.0))],
     [1.5, 2.0]),
    ("uniform", [((-1.0, 3.0), {}), ((), dict(loc=-1.0, scale=3.0)),
                 ((-1.0,), dict(scale=3.0))], [-1.0, 3.0]),
    ("expon", [((0.5, 2.0), {}), ((), dict(scale=2.0, loc=0.5)), ((0.5,), dict(scale=2.0))],
     [0.5, 2.0]),
    ("laplace", [((1.0, 0.5), {}), ((), dict(loc=1.0, scale=0.5)),
                 ((1.0,), dict(scale=0.5))], [1.0, 0.5]),
    ("lognorm", [((0.5, 0.0, 2.0), {}), ((), dict(s=0.5, scale=2.0)),
                 ((0.5,), dict(scale=2.0))], [0.5, 0.0, 2.0]),
    ("gamma", [((2.0, 1.0, 3.0), {}), ((), dict(a=2.0, loc=1.0, scale=3.0)),
               ((2.0, 1.0), dict(scale=3))], [2.0, 1.0, 3.0]),
    ("beta", [((2.0, 3.0, 1.0, 1.0), {}), ((), dict(a=2, b=3, loc=1)),
              ((2.0,), dict(b=3.0, loc=1.0))], [2.0, 3.0, 1.0, 1.0]),
]


@pytest.mark.parametrize("name,forms,want", _FAMILY_FORMS, ids=[f[0] for f in _FAMILY_FORMS])
def test_device_family_params_forms(name, forms, want):
    """RV.device_spec of every device family, built positionally, by keyword
    and mixed: the family's kind and [shape.., loc, scale] padded to 4, and
    those values reproduce the RV's own scipy log density (in the support,
    at its ends and outside)."""
    from pyabc_amd._native import PRIOR_KINDS as K
    for args, kwargs in forms:
        rv = pa.RV(name, *args, **kwargs)
        kind, par = rv.device_spec()
        assert kind == K[name] and len(par) == 4
        assert all(type(v) is float for v in par)
        assert par == [float(v) for v in want] + [0.0] * (4 - len(want)), (args, kwargs)
        lo, hi = rv.distribution.support()
        x = np.concatenate([rv.distribution.ppf([0.01, 0.3, 0.5, 0.9, 0.999]),
                            [lo, hi, max(lo, -1e300) - 1.0, min(hi, 1e300) + 1.0]])
        with np.errstate(divide="ignore", invalid="ignore"):
            np.testing.assert_array_equal(_spec_logpdf(name, par, x),
                                          rv.distribution.logpdf(x))
    # defaults: loc 0, scale 1
    shapes = want[:len(want) - 2]
    assert pa.RV(name, *shapes).device_spec() == \
        (K[name], [float(v) for v in shapes] + [0.0, 1.0] + [0.0] * (2 - len(shapes)))
    d = pa.Distribution(b=pa.RV(name, *forms[0][0]), a=pa.RV("norm", 0, 1))
    kinds, params = d.device_spec()
    assert kinds.dtype == np.int32 and list(kinds) == [K["norm"], K[name]]
    np.testing.assert_array_equal(params.reshape(2, 4)[1], pa.RV(name, *forms[0][0]).device_spec()[1])


def test_device_spec_never_a_wrong_family():
    """Distributions the kernels do not implement -- relatives of the device
    families, other parametrisations of them -- get the HOST spec (their
    support interval and a point inside it) or None, never a family's kind
    with parameters that mean something else."""
    from pyabc_amd._native import PRIOR_KINDS as K
    fam = {K[n] for n in ("norm", "uniform", "expon", "laplace", "lognorm", "gamma", "beta")}
    others = [pa.RV("halfnorm", 0, 1), pa.RV("truncnorm", -1, 2), pa.RV("invgamma", 2.0),
              pa.RV("gengamma", 2.0, 1.5), pa.RV("loggamma", 2.0), pa.RV("betaprime", 2, 3),
              pa.RV("loguniform", 1, 10), pa.RV("truncexpon", 3.0), pa.RV("laplace_asymmetric", 2),
              pa.RV("skewnorm", 1.0), pa.RV("chi2", 3), pa.RV("t", 3, loc=1),
              pa.RV("powerlognorm", 2.0, 0.5), pa.RV("erlang", 2)]
    for rv in others:
        spec = rv.device_spec()
        assert spec is None or spec[0] == K["host"], rv
        assert spec is None or spec[0] not in fam
        if spec is not None:
            lo, hi, c, _ = spec[1]
            assert (lo, hi) == tuple(float(v) for v in rv.distribution.support())
            assert lo <= c <= hi and np.isfinite(c) and rv.distribution.pdf(c) > 0
    # a family name whose frozen form the mapping cannot read back (an
    # unknown keyword cannot be frozen by scipy at all)
    with pytest.raises(TypeError):
        pa.RV("gamma", 2.0, rate=3.0)
    with pytest.raises(TypeError):
        pa.RV("gamma", scale=2.0)       # shape missing
    # a bounded HOST interval carries its centre
    assert pa.RV("truncnorm", -1, 2, loc=1).device_spec() == (K["host"], [0.0, 3.0, 1.5, 0.0])


def test_model_perturbation_kernel_checks():
    k = pa.ModelPerturbationKernel(3, probability_to_stay=.5)
    assert k.pmf(0, 0) == .5 and k.pmf(1, 0) == .25
    assert k.pmf(3, 0) == 0          # the reference's n == nr_of_models case
    with pytest.raises(Exception):
        k.pmf(4, 0)
    with pytest.raises(Exception):
        k.pmf(-1, 0)
    with pytest.raises(Exception):
        k.pmf(0, 3)


def test_integrated_model_accept():
    class M(pa.IntegratedModel):
        def integrated_simulate(self, pars, eps):
            d = abs(pars["x"] - 1)
            return pa.ModelResult(accepted=d <= eps, distance=d)
    res = M().accept(0, {"x": 1.2}, None, None, lambda t: 0.5, None, None)
    assert res.accepted and abs(res.distance - .2) < 1e-15
    with pytest.raises(NotImplementedError):
        pa.IntegratedModel().integrated_simulate({}, 1.0)
