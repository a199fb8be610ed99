"""Every entry of every compile-time dimension list, against the numpy oracle.

The kernels templated on a dimension are chosen by dispatch_int /
dispatch_candidate (abc_common.h, abc_candidate.h) from lists named next to
them: CandDims (proposals, fused round, regeneration), LocalDims, MomDims,
LseKBs, PackRanks, X3KBs.  The other suites reach a handful of entries; here
each entry and each list's fallback runs once, on the smallest shapes that
still cross a block edge.  The candidate path is compared with the oracle's
replay, not abc_candidates_propose with abc_propose: both go through one
dispatcher, so agreeing with each other would not tell a wrong entry from a
right one.  Tolerances are those of the entry's existing test
(tests/test_gpu_kernels.py), named at each use.
"""
import numpy as np
import pytest

import oracle
import oracle.sampler as osamp
from test_gpu_fused import T, _case, _check_equal, _round, _staged, dev  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# every d up to one past the largest CandDims entry, and the largest d of the
# register kernels (runtime-d instantiation D = 0 for d not in the list)
CAND_D = list(range(1, 18)) + [64]
MODES = ["mvn", "local", "prior"]
SEED, GEN = 11, 3          # _round's and _staged's defaults


def _bounded_case(d, mode):
    """N = 65 particles; coordinate 0 has a bounded prior, so that proposals
    from a population are re-drawn at every D."""
    kinds = ["uniform"] + ["norm"] * (d - 1)
    params = np.tile([0.0, 1.0, 0, 0], (d, 1))
    params[0] = [-1.5, 4.0, 0, 0]
    return _case(d, 1, N=65, mode=mode, seed=d, kinds=kinds, params=params)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", CAND_D + [65])
def test_proposals_every_dimension_vs_oracle(dev, d, mode):
    """gpu.propose (abc_propose / abc_local_propose) and CandidateRound.propose
    (abc_candidates_propose) at B = 257 (one full block and one ragged row):
    ancestors and attempts equal the oracle replay's, theta and the prior
    log-density to test_propose_replay's tolerances.  d = 65 is the wide
    kernel of abc_propose; the candidate kernels refuse it."""
    from pyabc_amd import gpu
    c = _bounded_case(d, mode)
    h = c["host"]
    lo, B = 1000, 257
    if mode == "prior":
        th_o, lp_o, att_o, _ = osamp.propose_prior(h["kinds"], h["params"], SEED, GEN, lo, B)
        anc_o = None
    else:
        fn = osamp.propose_local if mode == "local" else osamp.propose_mvn
        th_o, lp_o, anc_o, att_o = fn(h["X"], h["w"], h["L"], SEED, GEN, lo, B,
                                      h["kinds"], h["params"])
        assert (att_o > 1).any()     # re-draws happened
    got = [gpu.propose(c["X"], c["cdf"], c["L"], c["kind"], c["params"], SEED, GEN, lo, B,
                       1000, d, per_particle_L=c["ppl"], guide=c["guide"])]
    if d <= 64:
        got.append(_round(c).propose(lo, B))
    else:
        with pytest.raises(ValueError):
            _round(c)
    for th, lp, anc, att in got:
        if anc_o is not None:
            np.testing.assert_array_equal(anc.cpu().numpy(), anc_o)
        np.testing.assert_array_equal(att.cpu().numpy(), att_o)
        np.testing.assert_allclose(th.cpu().numpy(), th_o, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(lp.cpu().numpy(), lp_o, rtol=1e-12)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", CAND_D)
def test_fused_round_every_dimension(dev, d, mode):
    """abc_candidates_round + abc_candidates_regen at S = 5, B = 2049 (one
    tile and one tail candidate), p = 2 (the p2 kernels) and p = 3, plain and
    filter, eps at the staged distances' median: test_gpu_fused's
    _check_equal against the staged kernels."""
    lo, B = 1000, 2049
    for p in (2.0, 3.0):
        c = _case(d, 5, N=65, mode=mode, seed=d, p=p)
        eps = float(_staged(c, lo, B, np.inf)["dist"].median())
        ref = _staged(c, lo, B, eps)
        fr = _round(c)
        for filt in (False, True):
            assert _check_equal(c, fr, ref, lo, B, eps, filt) > 0


@pytest.mark.parametrize("d", range(1, 17))
def test_local_fit_and_logpdf_every_dimension(dev, d):
    """abc_local_fit and abc_local_logpdf at every LocalDims entry, N = 200,
    k = 20, M = 65: tolerances of test_local_fit_selection_paths_vs_oracle
    and test_local_logpdf_mfma_vs_oracle.  The density takes the oracle's
    fit, so each entry is checked on its own."""
    from pyabc_amd import gpu
    rng = np.random.default_rng(400 + d)
    N, k, M = 200, 20, 65
    X = rng.normal(size=(N, d))
    w = np.exp(0.3 * rng.standard_normal(N))
    w /= w.sum()
    ref = oracle.local_fit(X, w, k=k, k_fraction=None)
    covs, inv, dets, chol, lnorm = gpu.local_fit(T(X), T(w), k, 1.0, 1e-3)
    np.testing.assert_allclose(covs.cpu().numpy(), ref["covs"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(dets.cpu().numpy(), ref["dets"], rtol=1e-8)
    x = X[rng.integers(0, N, M)] + 0.1 * rng.normal(size=(M, d))
    lp_o = oracle.local_logpdf(x, X, ref)
    assert np.isfinite(lp_o).all()
    lp = gpu.local_logpdf(T(x), T(X), T(w), T(ref["inv_covs"]),
                          T(np.log(ref["normalization"]))).cpu().numpy()
    np.testing.assert_allclose(lp, lp_o, rtol=0, atol=2e-6)


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16])
def test_weighted_moments_every_dimension(dev, d):
    """abc_weighted_moments at every MomDims entry and d = 7 (the generic
    kernels), N = 300 (a full block and a ragged one): test_weighted_moments'
    tolerances."""
    from pyabc_amd import gpu
    rng = np.random.default_rng(500 + d)
    N = 300
    X = rng.standard_normal((N, d)) + 5
    w = rng.uniform(size=N)
    sw, sw2, mean, cov_b, wmax = gpu.weighted_moments(T(X), T(w), with_max=True)
    assert wmax == w.max()
    assert sw == pytest.approx(w.sum(), rel=1e-13)
    assert sw2 == pytest.approx((w ** 2).sum(), rel=1e-13)
    np.testing.assert_allclose(mean, w @ X / w.sum(), rtol=1e-13)
    np.testing.assert_allclose(cov_b * sw / (sw - sw2 / sw),
                               np.atleast_2d(np.cov(X, aweights=w, rowvar=False)),
                               rtol=1e-10, atol=1e-13)


# f64: mvn_lse_kernel<double, KB>, KB = ceil((r + 1) / 4) = 1 .. 15 (LseKBs).
# x3: pack_x3_kernel<., r> at every PackRanks entry and r = 11 (runtime r),
# mvn_x3_kernel<KB> at KB = 2 .. 11 (X3KBs; r = 14, 17, 19, 22, 25 are the
# first ranks of KB = 7 .. 11)
MVN_RANKS = ([("f64", 4 * kb - 1) for kb in range(1, 16)] +
             [("x3", r) for r in list(range(1, 13)) + [14, 16, 17, 19, 22, 25]])


@pytest.mark.parametrize("precision,d", MVN_RANKS)
def test_mvn_logpdf_every_rank(dev, precision, d):
    """The MFMA transition density of a full-rank population, N = 300,
    M = 65, against the fp64 oracle: 2e-6 (f64, test_mvn_pdf_golden) and 1e-6
    (x3 unhinted, test_mvn_x3_ranks_vs_oracle), relative, of the density."""
    import pandas as pd
    from pyabc_amd import _native as nat
    from pyabc_amd.transition import MultivariateNormalTransition
    rng = np.random.default_rng(600 + d)
    N, M = 300, 65
    X = 0.5 + 0.7 * rng.standard_normal((N, d))
    w = np.exp(0.3 * rng.standard_normal(N))
    w /= w.sum()
    cols = [f"p{k:02d}" for k in range(d)]
    t = MultivariateNormalTransition(precision=precision)
    t.fit(pd.DataFrame(X, columns=cols), w.copy())
    x = X[rng.integers(0, N, M)] + 0.3 * rng.standard_normal((M, d))
    lp = t.logpdf_device(T(x)).cpu().numpy()
    assert t._mfma and t._prec == {"f64": nat.ABC_PREC_F64, "x3": nat.ABC_PREC_X3}[precision]
    ref = oracle.mvn_logpdf(x, X, w, t.cov)
    np.testing.assert_allclose(np.exp(lp - ref), 1.0, rtol={"f64": 2e-6, "x3": 1e-6}[precision])
