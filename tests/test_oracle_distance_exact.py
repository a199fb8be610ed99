"""oracle/distance_exact.py against hand-worked rationals, numpy within numpy's
own bound, and the special-value table; and the conditions the device tests
(tests/test_gpu_distance_chain.py) put on their inputs, checked on the oracle
alone.  Host only."""
import math
from fractions import Fraction

import numpy as np
import pytest

import oracle
from oracle import distance_exact as dx

import distance_chain_ref as ref

U = dx.U
INF, NAN = math.inf, math.nan


def one(x, x0, wf, p):
    r = dx.pnorm_exact(np.array([x], dtype=np.float64), x0, wf, p)
    return float(r.d[0]), float(r.sum_p[0]), int(r.kind[0])


# ---- hand-worked rationals --------------------------------------------------------

def test_pythagorean_rows():
    ones = np.ones(2)
    assert one([3, 4], np.zeros(2), ones, 2.0)[:2] == (5.0, 25.0)
    assert one([3, 4], np.zeros(2), ones, 1.0)[:2] == (7.0, 7.0)
    assert one([3, -4], np.zeros(2), ones, INF)[:2] == (4.0, 4.0)
    # shifted and weighted: wf (x - x0) = (5, -12)
    assert one([3.5, -5.0], [1.0, 1.0], [2.0, 2.0], 2.0)[:2] == (13.0, 169.0)
    # 2-3-6-7 and 1-4-8-9
    assert one([2, 3, 6], np.zeros(3), np.ones(3), 2.0)[0] == 7.0
    assert one([1, 4, 8], np.zeros(3), np.ones(3), 2.0)[0] == 9.0
    # scaled far out of float64's squares: 3e200, 4e200 as powers of two
    a = 2.0 ** 600
    assert one([3 * a, 4 * a], np.zeros(2), ones, 2.0)[0] == 5 * a
    assert one([3 / a, 4 / a], np.zeros(2), ones, 2.0)[0] == 5 / a


def test_cubes_of_powers_of_two():
    # 1^3 + 2^3 * 7 = 57 ... use exact cubes: 3^3 + 4^3 + 5^3 = 6^3
    assert one([3, 4, 5], np.zeros(3), np.ones(3), 3.0)[:2] == (6.0, 216.0)
    # (2^a)^3 alone: the root is the power of two itself
    for a in (-300, -7, 0, 11, 300):
        assert one([2.0 ** a], [0.0], [1.0], 3.0)[0] == 2.0 ** a
    # eight equal terms 2^a: (8 2^3a)^(1/3) = 2^(a + 1)
    assert one([2.0 ** 5] * 8, np.zeros(8), np.ones(8), 3.0)[0] == 2.0 ** 6


def test_noninteger_p_by_hand():
    # p = 1.5: 4^1.5 + 9^1.5 = 8 + 27 = 35 -> 35^(2/3)
    d, s, _ = one([4, 9], np.zeros(2), np.ones(2), 1.5)
    assert s == 35.0
    assert d == pytest.approx(35.0 ** (2 / 3), rel=4 * U)
    # a single term is itself, for any p
    for p in (1.5, 2.5, 7.25):
        assert one([0.3], [0.0], [1.0], p)[0] == 0.3


@pytest.mark.parametrize("family", ["benign", "wide", "cancelling", "integers"])
def test_half_integer_roots_equal_mpmath(family):
    """p = 1.5 and 2.5: the integer square roots give what mpmath's pow per
    term gives -- the same float64 and the same rounding error to 1e-30."""
    for S in (1, 7, 65):
        x, x0, wf = ref.inputs(family, S, B=12)
        for p in (1.5, 2.5):
            a = dx.pnorm_exact(x, x0, wf, p)
            b = dx.pnorm_exact(x, x0, wf, p, half_integer_fast=False)
            assert np.array_equal(a.d, b.d) and np.array_equal(a.sum_p, b.sum_p)
            np.testing.assert_allclose(a.round_err, b.round_err, rtol=0, atol=1e-30)


def test_rounded_once_against_fractions():
    """p = 1 and inf: the float64 result is the Fraction sum / max rounded
    once; p = 2: its square brackets the exact sum between neighbours."""
    rng = np.random.default_rng(5)
    for S in (1, 3, 17):
        x = rng.standard_normal((6, S)) * 10 ** rng.uniform(-30, 30, S)
        x0 = rng.standard_normal(S)
        wf = rng.uniform(0.1, 2, S)
        r1, ri, r2 = (dx.pnorm_exact(x, x0, wf, p) for p in (1.0, INF, 2.0))
        for b in range(6):
            t = [abs(Fraction(float(wf[k])) * (Fraction(float(x[b, k])) - Fraction(float(x0[k]))))
                 for k in range(S)]
            s1 = sum(t)
            assert r1.d[b] == dx.ratio(s1.numerator, s1.denominator)
            assert ri.d[b] == dx.ratio(max(t).numerator, max(t).denominator)
            assert abs(Fraction(float(r1.d[b])) - s1) / s1 == \
                pytest.approx(abs(r1.round_err[b]), abs=1e-30)
            s2 = sum(v * v for v in t)
            lo, hi = (Fraction(float(np.nextafter(r2.d[b], s))) for s in (0.0, INF))
            assert lo * lo < s2 < hi * hi
            assert abs(r2.round_err[b]) <= U


@pytest.mark.parametrize("p", ref.P_LIST)
def test_against_numpy_on_benign_inputs(p):
    """numpy rounds each term twice, each power and each sum: within
    bound_u (the kernels' chain is numpy's, up to the summation order) + u for
    the oracle's own rounding."""
    for S in (1, 5, 33, 130):
        x, x0, wf = ref.inputs("benign", S, B=64)
        r = dx.pnorm_exact(x, x0, wf, p)
        got = oracle.pnorm(x, x0, w=wf, p=p)
        assert (r.kind == dx.FINITE).all()
        np.testing.assert_array_less(np.abs(got - r.d) / r.d / U,
                                     ref.bound_u(S, p, r.sum_p) + 1)


# ---- the special-value table --------------------------------------------------------

TABLE = [
    # x, x0, wf -> kind
    ([NAN, 1.0], [0.0, 0.0], [1.0, 1.0], dx.NAN),
    ([1.0, NAN], [0.0, 0.0], [1.0, 1.0], dx.NAN),          # a late NaN too
    ([1.0, 1.0], [0.0, NAN], [1.0, 1.0], dx.NAN),
    ([1.0, 1.0], [0.0, 0.0], [1.0, NAN], dx.NAN),
    ([INF, 1.0], [INF, 0.0], [1.0, 1.0], dx.NAN),          # inf - inf
    ([-INF, 1.0], [-INF, 0.0], [1.0, 1.0], dx.NAN),
    ([INF, 1.0], [0.0, 0.0], [0.0, 1.0], dx.NAN),          # 0 inf
    ([1.0, 1.0], [-INF, 0.0], [0.0, 1.0], dx.NAN),
    ([1.0, 1.0], [1.0, 0.0], [INF, 1.0], dx.NAN),          # inf 0
    ([INF, NAN], [0.0, 0.0], [1.0, 1.0], dx.NAN),          # NaN beats inf
    ([INF, 1.0], [0.0, 0.0], [1.0, 1.0], dx.INF),
    ([-INF, 1.0], [0.0, 0.0], [1.0, 1.0], dx.INF),
    ([INF, 1.0], [-INF, 0.0], [1.0, 1.0], dx.INF),         # inf - -inf
    ([1.0, 1.0], [INF, 0.0], [1.0, 1.0], dx.INF),
    ([2.0, 1.0], [1.0, 0.0], [INF, 1.0], dx.INF),
    ([1.0, 1.0], [0.0, 0.0], [1.0, 1.0], dx.FINITE),
]


@pytest.mark.parametrize("p", ref.P_LIST)
def test_special_value_table(p):
    for x, x0, wf, kind in TABLE:
        d, s, k = one(x, np.array(x0), np.array(wf), p)
        assert k == kind, (x, x0, wf)
        if kind == dx.NAN:
            assert math.isnan(d) and math.isnan(s)
        elif kind == dx.INF:
            assert d == INF and math.isnan(s)
        else:
            assert math.isfinite(d) and s > 0


@pytest.mark.parametrize("p", ref.P_LIST)
def test_negative_zero_is_zero(p):
    z = -0.0
    assert one([z, 0.0, 2.0], [0.0, z, 2.0], [1.0, z, z], p) == (0.0, 0.0, dx.FINITE)
    assert math.copysign(1.0, one([z], [0.0], [z], p)[0]) == 1.0
    assert one([z, 3.0], [0.0, 0.0], [1.0, 1.0], p)[0] == 3.0


def test_rows_are_independent():
    x, x0, wf = ref.special_case("x_nan", 5, 2)
    r = dx.pnorm_exact(x, x0, wf, 2.0)
    rows = ref.special_rows()
    assert (r.kind[rows] == dx.NAN).all()
    keep = np.setdiff1d(np.arange(len(x)), rows)
    assert np.array_equal(r.d[keep], dx.pnorm_exact(x[keep], x0, wf, 2.0).d)


def test_overflow_and_underflow_of_the_result_only():
    big, ones = 2.0 ** 1023, np.ones(2)
    assert one([big, big], np.zeros(2), ones, 2.0)[0] == big * math.sqrt(2)   # fits
    assert one([big, big], np.zeros(2), ones, 1.0)[0] == INF                  # 2^1024
    assert one([1e200, 1.0], np.zeros(2), ones, 2.0)[0] == 1e200              # numpy: inf
    assert one([1e-170, 1e-170], np.zeros(2), ones, 2.0)[0] == \
        pytest.approx(math.sqrt(2) * 1e-170, rel=2 * U)                       # numpy: 0


# ---- the accept reference ----------------------------------------------------------------

def test_accept_exact_never_takes_nan():
    d = np.array([NAN, -0.0, 0.0, 5e-324, 1.0, INF])
    assert dx.accept_exact(d, INF).tolist() == [1, 2, 3, 4, 5]
    assert dx.accept_exact(d, 1.0).tolist() == [1, 2, 3, 4]
    assert dx.accept_exact(d, -0.0).tolist() == [1, 2]
    assert dx.accept_exact(d, -1.0).tolist() == []
    assert dx.accept_exact(d, NAN).tolist() == []


def test_undecidable_set_by_hand():
    # distances 1, 1 + 2^-40, 2, inf, NaN against eps = 1 and a 2^-30 bound
    x = np.array([[1.0], [1.0 + 2.0 ** -40], [2.0], [INF], [NAN]])
    r = dx.pnorm_exact(x, np.zeros(1), np.ones(1), 1.0)
    assert dx.undecidable(r, 1.0, 2.0 ** -30).tolist() == [True, True, False, False, False]
    assert dx.undecidable(r, 1.0, 2.0 ** -50).tolist() == [True, False, False, False, False]
    assert dx.accepted_exact(r, 1.0).tolist() == [True, False, False, False, False]
    assert dx.accepted_exact(r, INF).tolist() == [True, True, True, True, False]


# ---- conditions on the device tests' inputs ---------------------------------------------------

def test_wide_family_stays_inside_the_exponent_range():
    """|term|^p within [2^-900, 2^900] for p <= 3: nothing over- or underflows
    in the kernels and the exact result is representable."""
    for S in ref.S_LIST:
        x, x0, wf = ref.inputs("wide", S)
        t = np.abs(wf * (x - x0))
        assert t.min() > 2.0 ** -299 and t.max() < 2.0 ** 299, S


def test_cancelling_family_differences_are_exact():
    for S in (1, 33):
        x, x0, wf = ref.inputs("cancelling", S, B=50)
        for b in range(50):
            for k in range(S):
                assert Fraction(float(x[b, k] - x0[k])) == \
                    Fraction(float(x[b, k])) - Fraction(float(x0[k]))
        assert np.abs(x - x0).max() < 1e-9 * np.abs(x0).max()


DECISION_S = [2, 32, 33, 129]


@pytest.mark.parametrize("family", ["benign", "wide"])
def test_decision_inputs_are_decidable(family):
    """eps = the exact median distance: at most 1 % of the rows lie within the
    kernels' bound of it (the condition of test_decisions_against_exact)."""
    for S in DECISION_S:
        for p in ref.P_LIST:
            r = ref.reference(family, S, p)
            eps = float(np.median(r.d))
            und = dx.undecidable(r, eps, ref.bound_u(S, p, r.sum_p) * U)
            assert 1 <= und.sum() <= 0.01 * len(r.d), (S, p, und.sum())
