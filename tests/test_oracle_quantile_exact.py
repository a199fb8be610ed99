"""The exact weighted-quantile reference (oracle/quantile_exact.py) on the
host: its dyadic weights are what they claim, its rules are np.interp's, and
the float64 numpy oracle satisfies both rules of the tolerance model
(tests/test_gpu_quantile.py) on every input recipe the device tests use --
the model has to be satisfiable by the reference alone before a kernel is
held to it.
"""
import numpy as np
import pytest

import oracle
import oracle.quantile_exact as qe

N_ONE, N_FOUR = 36_865, (1 << 20) + 1


@pytest.mark.parametrize("kind", ["flat", "skew", "dominant", "zeros"])
@pytest.mark.parametrize("N", [1, 2, 4097, N_FOUR])
def test_dyadic_weights_sum_exactly(kind, N):
    """Any order of summation gives the same float64 partial sums as the
    80-bit ones, and the total is exactly 1."""
    rng = qe.seed(f"dyadic:{kind}:{N}")
    w, m, k = qe.dyadic_weights(rng, N, kind)
    assert m.dtype == np.int64 and int(m.sum()) == 1 << k and k < 53
    assert np.array_equal(w * float(1 << k), m.astype(np.float64))
    cs = np.cumsum(w)
    assert np.array_equal(cs.astype(np.longdouble), np.cumsum(w.astype(np.longdouble)))
    assert cs[-1] == 1.0
    for _ in range(2):
        assert np.cumsum(w[rng.permutation(N)])[-1] == 1.0
    assert float(np.sum(w)) == 1.0                       # numpy's pairwise tree
    half = cs - 0.5 * w
    assert np.array_equal(half.astype(np.longdouble),
                          np.cumsum(w.astype(np.longdouble)) - w.astype(np.longdouble) / 2)


def test_dyadic_edge_zeros_and_dominant_places():
    rng = qe.seed("places")
    pts = rng.gamma(2.0, 1.5, 5000)
    order = np.argsort(pts, kind="stable")
    _, m, _ = qe.dyadic_weights(rng, 5000, "edge_zeros", points=pts)
    assert not m[order[:50]].any() and not m[order[-50:]].any()
    assert (m[order[50:-50]] > 0).all()
    _, m, k = qe.dyadic_weights(rng, 5000, "dominant", points=pts)
    assert int(np.argmax(m)) == order[2500] and k == 41
    assert np.count_nonzero(m == 1) == 4999


def interp(pts, w, alpha):
    with np.errstate(invalid="ignore"):
        return oracle.weighted_quantile(pts, w, alpha, kind="stable")


def test_rules_on_four_points():
    """Clamps, an exact knot, inf - inf, equal xp from zero weights, no
    positive weight: hand-made values, and np.interp's own answer."""
    p = np.array([3.0, 1.0, 4.0, 2.0])
    m = np.array([1, 1, 1, 1])                 # xp = .125 .375 .625 .875
    for a, q, clamp, copy in [(0.05, 1.0, True, True), (0.95, 4.0, True, True),
                              (0.0, 1.0, True, True), (1.0, 4.0, True, True),
                              (0.375, 2.0, False, True), (0.875, 4.0, False, True),
                              (0.5, 2.5, False, False), (0.125, 1.0, False, True)]:
        r = qe.weighted_quantile_exact(p, m, a)
        assert (r.q, r.clamp, r.copy) == (q, clamp, copy), a
        assert r.q == interp(p, m / 4, a)
    r = qe.weighted_quantile_exact(p, m, 0.5)
    assert (float(r.xj), float(r.xj1), r.yj, r.yj1, r.j) == (0.375, 0.625, 2.0, 3.0, 1)
    # unnormalised float weights: the division by the total is the reference's
    assert qe.weighted_quantile_exact(p, 7.0 * np.ones(4), 0.5).q == 2.5
    # inf - inf inside the run, finite -> inf across its start
    p = np.array([np.inf, 1.0, np.inf, 2.0])
    for a, q in [(0.75, np.inf), (0.5, np.inf), (0.375, 2.0), (0.625, np.inf),
                 (0.25, 1.5), (1.0, np.inf)]:
        r = qe.weighted_quantile_exact(p, m, a)
        assert r.q == q and r.q == interp(p, m / 4, a), a
    # zero weights: xp = .125 .25 .25 .625 -- the last of the equal knots
    p = np.array([1.0, 2.0, 3.0, 4.0])
    m = np.array([1, 0, 0, 3])
    for a, q in [(0.25, 3.0), (0.1875, 1.5), (0.4375, 3.5), (0.125, 1.0)]:
        r = qe.weighted_quantile_exact(p, m, a)
        assert r.q == q and r.q == interp(p, m / 4, a), a
    # zero weights at both ends: alpha = 0 sits on the equal knots at 0 and
    # takes the last of them, alpha = 1 takes the last point
    m = np.array([0, 0, 4, 0])
    assert qe.weighted_quantile_exact(p, m, 0.0).q == 2.0 == interp(p, m / 4, 0.0)
    assert qe.weighted_quantile_exact(p, m, 1.0).q == 4.0 == interp(p, m / 4, 1.0)
    # ties: the stable order decides whose weight comes first
    p = np.array([1.0, 1.0, 2.0, 2.0])
    m = np.array([1, 5, 1, 1])
    r = qe.weighted_quantile_exact(p, m, 0.625)  # xp = 1/16 7/16 13/16 15/16
    assert r.j == 1 and r.q == 1.5 == interp(p, m / 8, 0.625)
    # -0.0 and +0.0 are one value
    r = qe.weighted_quantile_exact(np.array([0.0, -0.0, 0.0, -0.0]), np.ones(4, int), 0.4)
    assert r.q == 0.0
    # no positive weight: no knots
    for w in (np.zeros(4, int), np.zeros(4)):
        assert np.isnan(qe.weighted_quantile_exact(p, w, 0.5).q)


def extra_alphas(case, ref, m):
    if case == "inf30":
        return qe.inf_alphas(ref)
    if case == "dominant":
        return qe.dominant_alphas(ref, m)
    if case == "staircase":
        return qe.staircase_alphas(ref)
    return ()


DYADIC = list(qe.SHAPE_CASES) + list(qe.KEY_CASES) + list(qe.WEIGHT_CASES)


@pytest.mark.parametrize("N", [N_ONE, N_FOUR])
@pytest.mark.parametrize("case", DYADIC)
def test_float64_oracle_within_dyadic_rule(case, N):
    """Dyadic weights: numpy's float64 cumsum + interp and the exact reference
    agree to 2 ulp of the larger knot value (half the kernels' allowance), and
    exactly where q is a copy of an input point or infinite."""
    pts, w, m = qe.dyadic_case(case, N)
    ref = qe.ExactQuantile(pts, m)
    assert np.array_equal(ref.xp.astype(np.float64).astype(np.longdouble), ref.xp)
    alphas = qe.alpha_set(ref, extra=extra_alphas(case, ref, m))
    got = interp(pts, w, np.array(alphas))
    for a, q in zip(alphas, got):
        r = ref(a)
        tol = qe.budget_dyadic(r) / 2
        if tol == 0.0:
            assert qe.same_value(q, r.q), (case, a, q, r)
        else:
            assert abs(q - r.q) <= tol, (case, a, q, r, abs(q - r.q) / qe.ulp_max(r))
    if case == "inf30":
        inside, last_finite, first_inf, mid = [ref(a) for a in alphas[-4:]]
        assert inside.q == first_inf.q == mid.q == np.inf
        assert np.isfinite(last_finite.q) and last_finite.copy
    if case == "edge_zeros":
        assert ref(0.0).q == ref.p[49] and ref(1.0).q == ref.p[-1]


@pytest.mark.parametrize("N", [N_ONE, N_FOUR])
@pytest.mark.parametrize("case", list(qe.GENERAL_CASES) + ["ones"])
def test_float64_oracle_within_general_rule(case, N):
    """General weights: the float64 oracle stays inside 1e-12 |q| + N eps
    |dy| / dxp around the exact reference, and uses a small share of it."""
    if case == "ones":
        pts = qe.points_recipe(qe.seed(f"ones:{N}"), N, "normal")
        w = np.ones(N)
        ref = qe.ExactQuantile(pts, w)
        w = w / N
    else:
        pts, w = qe.general_case(case, N)
        ref = qe.ExactQuantile(pts, w)
    alphas = qe.alpha_set(ref, exact_knots=(case == "ones"))
    if case.startswith("two_cluster"):
        g = int(np.searchsorted(ref.p, 500.0))           # the gap's midpoint
        alphas.append((ref.knot(g - 1) + ref.knot(g)) / 2)
    got = interp(pts, w, np.array(alphas))
    worst = 0.0
    for a, q in zip(alphas, got):
        r = ref(a)
        tol, _ = qe.budget_general(r, N)
        assert abs(q - r.q) <= tol, (case, a, q, r)
        if tol > 0:
            worst = max(worst, abs(q - r.q) / tol)
    # the sequential cumsum of N equal weights rounds the same way at every
    # step, so "ones" uses up to 0.08 of the budget just below the last knot;
    # the others stay under 4e-3
    print(f"share of the general budget used by the float64 oracle: {case} N={N} "
          f"{worst:.2e}")
