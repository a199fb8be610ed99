"""Integer parameters, the host side: grid tables of discrete priors against
scipy, the refusals and their reasons, GenerationSpec.why_not, argument
checks of the C ABI (no device), the replay's displacement law, and the host
density against the reference's (tests/golden/randomwalk.npz)."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.stats as st

import walk_ref
from conftest import GOLDEN


def _frozen_rv(frozen):
    """An RV around an already frozen scipy distribution."""
    import pyabc_amd as pa
    rv = pa.RV("poisson", 1)
    rv.name, rv.args, rv.kwargs, rv.distribution = "frozen", (), {}, frozen
    return rv


CASES = {
    "poisson3": (lambda: st.poisson(3), 224),
    "poisson1000": (lambda: st.poisson(1000), 2374),
    "binom": (lambda: st.binom(50, .3), 51),
    "nbinom": (lambda: st.nbinom(5, .1), 7271),
    "geom": (lambda: st.geom(.01), 73683),
    "randint": (lambda: st.randint(0, 4), 4),
    "values": (lambda: st.rv_discrete(values=([0, 2], [.25, .75]))(), 3),
    "poisson3_shifted": (lambda: st.poisson(3, loc=-2), 224),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_grid_spec_window_and_tables(name):
    make, length = CASES[name]
    frozen = make()
    spec, why = _frozen_rv(frozen).grid_spec()
    assert why == "" and spec is not None
    k_lo, pmf, logpmf = spec
    assert len(pmf) == len(logpmf) == length
    ks = np.arange(k_lo, k_lo + length)
    # the window: first to last integer of positive float64 mass
    assert pmf[0] > 0 and pmf[-1] > 0
    assert frozen.pmf(k_lo - 1) == 0 and frozen.pmf(k_lo + length) == 0
    far = np.concatenate([np.arange(k_lo - 2000, k_lo), k_lo + length + np.arange(2000)])
    assert not (frozen.pmf(far) > 0).any()
    # the tables are scipy's bits
    assert np.array_equal(pmf, frozen.pmf(ks))
    pos = pmf > 0
    assert np.array_equal(logpmf[pos], frozen.logpmf(ks)[pos])
    assert np.all(logpmf[~pos] == -np.inf)
    if name == "values":
        assert k_lo == 0 and list(pos) == [True, False, True]
    if name == "poisson3_shifted":
        assert k_lo == -2
        assert np.array_equal(pmf, _frozen_rv(st.poisson(3)).grid_spec()[0][1])


def test_grid_spec_through_rv_names():
    import pyabc_amd as pa
    spec, why = pa.RV("binom", 50, .3).grid_spec()
    assert why == "" and spec[0] == 0 and len(spec[1]) == 51
    prior = pa.Distribution(b=pa.RV("randint", 0, 4), a=pa.RV("poisson", 3))
    specs, why = prior.grid_spec()
    assert why == "" and [len(s[1]) for s in specs] == [224, 4]   # sorted names
    assert prior.device_spec() is None


def test_grid_spec_refusals_name_the_reason():
    import pyabc_amd as pa
    spec, why = pa.RV("poisson", 3, loc=0.5).grid_spec()
    assert spec is None and "non-integer loc" in why
    spec, why = pa.RV("geom", 1e-6).grid_spec()
    assert spec is None and "2^20" in why
    spec, why = pa.RV("rv_discrete", values=([0, 1], [.5, .5])).grid_spec()
    assert spec is None and "not a frozen" in why
    spec, why = pa.LowerBoundDecorator(pa.RV("poisson", 3), 0).grid_spec()
    assert spec is None and "RVDecorator" in why
    spec, why = pa.RV("norm", 0, 1).grid_spec()
    assert spec is None and "continuous" in why
    specs, why = pa.Distribution(k=pa.RV("poisson", 3), x=pa.RV("norm", 0, 1)).grid_spec()
    assert specs is None and why == "x: continuous distribution"


# ---- GenerationSpec.why_not -----------------------------------------------------

class _History:
    def model_probabilities_dict(self, t=None):
        return {0: 0.5, 1: 0.5}


def _abc(priors, transitions=None, M=1):
    import pyabc_amd as pa
    models = [pa.VectorizedModel(lambda th, seed, gen, idx0: th[:, :1], ["y"])
              for _ in range(M)]
    kw = {} if transitions is None else dict(transitions=transitions)
    abc = pa.ABCSMC(models if M > 1 else models[0], priors if M > 1 else priors[0],
                    pa.PNormDistance(p=2), population_size=100,
                    sampler=pa.BatchedGPUSampler(), **kw)
    abc.x_0 = {"y": 0.0}
    abc.history = _History()
    return abc


def test_why_not_names_the_discrete_pieces():
    import pyabc_amd as pa
    grid = lambda: pa.Distribution(k=pa.RV("poisson", 3))

    spec = pa.GenerationSpec(_abc([grid()]), 1)     # default transition: MVN
    assert not spec.batched_capable
    assert "grid prior with a transition that is not a DiscreteRandomWalkTransition" \
        in spec.why_not

    spec = pa.GenerationSpec(_abc([pa.Distribution(k=pa.RV("norm", 0, 1))],
                                  pa.DiscreteRandomWalkTransition()), 1)
    assert not spec.batched_capable
    assert "DiscreteRandomWalkTransition with a continuous prior" in spec.why_not

    spec = pa.GenerationSpec(_abc([pa.Distribution(k=pa.RV("poisson", 3, loc=0.5))]), 0)
    assert not spec.batched_capable
    assert "without a grid form (k: non-integer loc 0.5)" in spec.why_not

    spec = pa.GenerationSpec(_abc([grid()], pa.DiscreteRandomWalkTransition(n_steps=600)), 1)
    assert not spec.batched_capable and "n_steps = 600 outside 1 .. 512" in spec.why_not

    wide = pa.Distribution(**{f"k{i:02d}": pa.RV("poisson", 3) for i in range(33)})
    spec = pa.GenerationSpec(_abc([wide], pa.DiscreteRandomWalkTransition()), 1)
    assert not spec.batched_capable and "over 33 parameters (1 .. 32)" in spec.why_not

    # a host fit is the numpy form: the generation stays per candidate
    spec = pa.GenerationSpec(_abc([grid()], pa.DiscreteRandomWalkTransition()), 1)
    assert not spec.batched_capable and "not fitted on the device" in spec.why_not

    spec = pa.GenerationSpec(_abc([grid(), grid()], M=2), 0)
    assert not spec.batched_capable
    assert "prior of model 0 is a grid prior (several models)" in spec.why_not


# ---- C ABI argument checks (no device) ----------------------------------------------

def test_walk_entries_validate_before_any_device_call():
    import ctypes as C
    from pyabc_amd import _native as nat
    lib = nat.load()
    fake = 4096     # never dereferenced: every check below fails first

    def code(name, *args):
        return getattr(lib, name)(*args)

    assert code("abc_walk_logpmf", fake, 10, fake, fake, 10, 33, fake, 1, fake, fake,
                1 << 20, None) == nat.ABC_ERR_UNSUPPORTED
    assert b"walk_logpmf" in lib.abc_last_error()
    assert code("abc_walk_logpmf", fake, 10, fake, fake, 10, 2, fake, 513, fake, fake,
                1 << 20, None) == nat.ABC_ERR_UNSUPPORTED
    assert code("abc_walk_logpmf", fake, 10, fake, fake, 0, 2, fake, 1, fake, fake,
                1 << 20, None) == nat.ABC_ERR_INVALID
    assert code("abc_walk_logpmf", None, 10, fake, fake, 10, 2, fake, 1, fake, fake,
                1 << 20, None) == nat.ABC_ERR_INVALID
    need = nat.query("abc_walk_logpmf_bytes", 10, 10, 2)
    assert code("abc_walk_logpmf", fake, 10, fake, fake, 10, 2, fake, 1, fake, fake,
                need - 1, None) == nat.ABC_ERR_WORKSPACE
    assert code("abc_walk_pack", fake, 10, 33, fake, fake, None) == nat.ABC_ERR_UNSUPPORTED
    assert code("abc_walk_pack", fake, 10, 2, fake, None, None) == nat.ABC_ERR_INVALID
    prop = lambda d, n, last, B=10, prior=None, att=5: code(
        "abc_walk_propose", fake, fake, None, 10, d, fake, n, last, prior, 1, 0, 0, B, att,
        fake, fake, fake, fake, None)
    assert prop(33, 1, 2) == nat.ABC_ERR_UNSUPPORTED
    assert prop(2, 513, 2) == nat.ABC_ERR_UNSUPPORTED
    assert prop(2, 1, 3) == nat.ABC_ERR_INVALID          # law_last > 2 n
    assert prop(2, 1, 2, att=0) == nat.ABC_ERR_INVALID
    bad = nat.GridPrior(3, fake, fake, fake)
    assert prop(2, 1, 2, prior=C.addressof(bad)) == nat.ABC_ERR_INVALID   # d differs
    assert b"prior d differs" in lib.abc_last_error()
    null = nat.GridPrior(2, fake, None, fake)
    assert code("abc_grid_prior_logpmf", fake, 10, C.addressof(null), fake, None) \
        == nat.ABC_ERR_INVALID
    assert code("abc_grid_prior_logpmf", fake, 10, None, fake, None) == nat.ABC_ERR_INVALID
    assert code("abc_grid_prior_draw", None, 1, 0, 0, 10, fake, None) == nat.ABC_ERR_INVALID
    wide = nat.GridPrior(65, fake, fake, fake)
    assert code("abc_grid_prior_draw", C.addressof(wide), 1, 0, 0, 10, fake, None) \
        == nat.ABC_ERR_INVALID
    # empty calls succeed without a device
    ok = nat.GridPrior(2, fake, fake, fake)
    assert code("abc_grid_prior_draw", C.addressof(ok), 1, 0, 0, 0, None, None) == nat.ABC_OK
    assert prop(2, 1, 2, B=0) == nat.ABC_OK
    assert code("abc_walk_logpmf", None, 0, None, None, 10, 2, None, 1, None, None, 0,
                None) == nat.ABC_OK


def test_walk_chunks_depend_on_the_shape_alone():
    from pyabc_amd import _native as nat
    lib = nat.load()
    for M, N, d in [(1, 1, 1), (1, 769, 2), (257, 4097, 5), (10 ** 5, 10 ** 5, 5),
                    (10 ** 6, 10 ** 6, 2), (1, 10 ** 6, 32)]:
        c = lib.abc_walk_logpmf_chunk(M, N, d)
        assert c == lib.abc_walk_logpmf_chunk(M, N, d) and c > 0 and c % 256 == 0
        chunks = -(-N // c)
        assert 1 <= chunks <= 256
        assert nat.query("abc_walk_logpmf_bytes", M, N, d) >= chunks * M * 8
    assert -(-769 // lib.abc_walk_logpmf_chunk(1, 769, 2)) >= 3
    assert lib.abc_walk_logpmf_chunk(10 ** 6, 10 ** 6, 2) >= 10 ** 6   # M fills the chip


# ---- the displacement law ---------------------------------------------------------

LAWS = [(1, 1. / 3, 1. / 3, 1. / 3), (3, .25, .35, .4), (4, .5, .5, 0.), (7, .2, .5, .3),
        (2, 0., .5, .5)]


@pytest.mark.parametrize("setting", LAWS)
def test_step_law_is_the_convolution_of_single_steps(setting):
    from pyabc_amd.transition.randomwalk import walk_step_law
    n = setting[0]
    law = walk_step_law(*setting)
    exact = walk_ref.exact_step_law(*setting)
    assert len(law) == len(exact) == 2 * n + 1
    for got, want in zip(law, exact):
        assert (got == 0) == (want == 0)          # e.g. the parity gaps at p_c = 0
        assert abs(got - float(want)) <= 1e-14 * float(want)


@pytest.mark.parametrize("setting", LAWS)
def test_replay_draws_the_law_at_every_threshold(setting):
    """The inverse CDF of the replay (and the kernel): the u-interval that
    draws index i is [cum[i-1], cum[i]) / cum[-1], checked at the doubles
    next to every threshold; an entry of law 0 is never drawn."""
    from pyabc_amd.transition.randomwalk import walk_step_law
    law = walk_step_law(*setting)
    cum, last = np.cumsum(law), walk_ref.last_positive(law)
    total = cum[-1]
    draw = lambda u: int(walk_ref.displacement_index(u, cum, last))
    positive = [i for i in range(len(law)) if law[i] > 0]
    assert draw(0.0) == positive[0]
    assert draw(1.0 - 2.0 ** -53) == positive[-1]
    for a, b in zip(positive[:-1], positive[1:]):
        # the largest u whose target is still below cum[a], and the next one
        u = cum[a] / total
        while u * total >= cum[a]:
            u = np.nextafter(u, 0.0)
        assert draw(u) == a
        assert draw(np.nextafter(u, 1.0)) == b
        # the interval's length is the law's entry
        lo = cum[a - 1] / total if a > positive[0] else 0.0
        assert abs((u - lo) - law[a] / total) <= 4 * 2.0 ** -53
    us = np.random.default_rng(3).random(20000)
    assert set(np.unique(walk_ref.displacement_index(us, cum, last))) <= set(positive)


# ---- host density against the reference's ---------------------------------------------

def test_host_pdf_equals_reference_golden():
    import pyabc_amd as pa
    g = np.load(os.path.join(GOLDEN, "randomwalk.npz"))
    X = pd.DataFrame(g["X"], columns=["a", "b"])
    x = pd.DataFrame(g["x"], columns=["a", "b"])
    assert g["pdf"].shape == (3, 30) and np.isfinite(g["pdf"]).all()
    for (n, p_l, p_r, p_c), want in zip(g["settings"], g["pdf"]):
        tr = pa.DiscreteRandomWalkTransition(n_steps=int(n), p_l=p_l, p_r=p_r, p_c=p_c)
        tr.fit(X, g["w"].copy())
        got = tr.pdf(x)
        assert np.array_equal(got == 0, want == 0) and (want == 0).any()
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        # the exact rational mass of the same tables agrees too
        exact = [float(f) for f in walk_ref.exact_mass(g["x"], g["X"], g["w"], tr._law())]
        np.testing.assert_allclose(got, exact, rtol=1e-13, atol=0)
