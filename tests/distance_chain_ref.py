"""Inputs, bounds and cached exact references shared by
tests/test_oracle_distance_exact.py (CPU) and tests/test_gpu_distance_chain.py.

Everything here is derived from the seed and the shape alone; nothing reads a
kernel's output.  u = 2^-53 (unit roundoff), as in oracle/weights_exact.py.
"""
import math
import zlib

import numpy as np

from oracle import distance_exact as dx

U = dx.U
S_LIST = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 700]
B_LIST = [1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 1037]
P_LIST = [1.0, 1.5, 2.0, 3.0, math.inf]
FAMILIES = ["benign", "wide", "cancelling", "dominant", "integers"]
BMAX = max(B_LIST)

# ulps of one device pow(double, double).  No document shipped with the
# toolchain states a figure, so it is measured ("The distance
# chain against exact references"): 88 039 distinct |term| values of the
# families below (16 rows of every S), fed as single-column rows, give
# d = pow(pow(a, p), fl(1 / p)), which mpmath's (a^p)^(fl(1 / p)) measures.
# Two calls with K ulps each (1 ulp <= 2 u) leave 2 (1 / p + 1) K u; the
# largest error seen was 2.86 u at p = 1.5 and 2.48 u at p = 3, that is
# K = 0.859 and 0.931.  The bound uses four times the larger.
K_POW_MEASURED = 0.931
K_POW = 4 * K_POW_MEASURED


def seed(*key):
    return zlib.crc32("-".join(str(k) for k in key).encode())


def inputs(family, S, B=BMAX):
    """x [B, S], x0 [S], wf [S] of one input family."""
    rng = np.random.default_rng(seed(family, S))
    if family == "benign":
        x = rng.standard_normal((B, S)) * 10 ** rng.uniform(-2, 2, S)
        return x, rng.standard_normal(S), rng.uniform(0.1, 2.0, S)
    if family == "wide":
        # columns over 80 decades, weights over 20: |term| within 10^+-55 or
        # so, |term|^3 within 2^+-900 (checked by the CPU test)
        c = 10 ** rng.uniform(-40, 40, S)
        return (c * rng.standard_normal((B, S)), c * rng.standard_normal(S),
                10 ** rng.uniform(-10, 10, S))
    if family == "cancelling":
        # x = x0 (1 + k 2^-52): x - x0 is exact (Sterbenz) and ~1e-13 |x0|
        x0 = rng.standard_normal(S) * 10 ** rng.uniform(-3, 3, S)
        k = rng.integers(-4096, 4097, (B, S)).astype(np.float64)
        return x0 * (1.0 + k * 2.0 ** -52), x0, rng.uniform(0.1, 2.0, S)
    if family == "dominant":
        x = rng.standard_normal((B, S)) * 10 ** rng.uniform(-2, 2, S)
        x0 = rng.standard_normal(S)
        j = S // 2
        x[:, j] = x0[j] + 1e8 * rng.uniform(1, 2, B) * rng.choice([-1.0, 1.0], B)
        return x, x0, rng.uniform(0.1, 2.0, S)
    if family == "integers":
        x = rng.integers(-20, 21, (B, S)).astype(np.float64)
        x0 = rng.integers(-20, 21, S).astype(np.float64)
        wf = rng.integers(0, 4, S).astype(np.float64)
        wf[0] = max(wf[0], 1.0)
        return x, x0, wf
    raise ValueError(family)


_cache = {}


def reference(family, S, p):
    """pnorm_exact of inputs(family, S), once per process; rows [:B] are the
    reference of the first B rows (rows are independent)."""
    key = (family, S, float(p))
    if key not in _cache:
        _cache[key] = dx.pnorm_exact(*inputs(family, S), p)
    return _cache[key]


def bound_u(S, p, sum_p=None):
    """The kernels' error bound relative to the exact distance, in units of u,
    to first order (derivation: tests/test_gpu_distance_chain.py).  sum_p [B]
    is needed for a general p only (|ln sum_p| enters through the rounded
    exponent 1/p)."""
    if p == math.inf:
        return 2.0
    if p == 1.0:
        return S + 2.0
    if p == 2.0:
        return (S + 3.0) / 2 + 1
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = np.where(np.asarray(sum_p) > 0, np.abs(np.log(sum_p)), 0.0)
    return (2 * p + 2 * K_POW + S - 1) / p + ln / p + 2 * K_POW


def rel_err_u(got, ref):
    """(got - exact) / exact in units of u for the FINITE rows of ref with a
    nonzero distance (0 elsewhere; those rows are compared as bits)."""
    got = np.asarray(got, dtype=np.float64)
    d = ref.d
    ok = (ref.kind == dx.FINITE) & (d != 0) & np.isfinite(d)
    with np.errstate(all="ignore"):
        e = (got - d) / d + ref.round_err
    return np.where(ok, e / U, 0.0), ok


def bits(a):
    """float64 -> uint64 bit patterns with every NaN mapped to one pattern."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7FF8000000000000)
    return b


# ---- special values ------------------------------------------------------------

SPECIAL_S = [5, 32, 33, 130]
SPECIAL_KINDS = ["x_nan", "x_pinf", "x_ninf", "x_x0_inf", "wf0_x_inf", "x0_nan",
                 "neg_zero"]
SPECIAL_B = 9            # wide rows: one full wave of PNORM_ROWS = 8 and one row more


def special_columns(S):
    cols = {0, S // 2, S - 1}
    if S > 64:
        cols.add(64)     # the second trip of the lane-strided loop
    return sorted(cols)


def special_rows(B=SPECIAL_B):
    return [0, B // 2, B - 1]


def special_case(kind, S, col, B=SPECIAL_B):
    """One matrix of small integers (p in {1, 2, inf} stay exact) with the
    special value in column ``col`` of rows 0, B // 2 and B - 1."""
    x, x0, wf = inputs("integers", S, B)
    wf = np.maximum(wf, 1.0)
    rows = special_rows(B)
    if kind == "x_nan":
        x[rows, col] = np.nan
    elif kind == "x_pinf":
        x[rows, col] = np.inf
    elif kind == "x_ninf":
        x[rows, col] = -np.inf
    elif kind == "x_x0_inf":      # the other rows: finite - inf, an infinite term
        x0[col] = np.inf
        x[rows, col] = np.inf
    elif kind == "wf0_x_inf":     # the other rows: 0 x finite
        wf[col] = 0.0
        x[rows, col] = [np.inf, -np.inf, np.inf]
    elif kind == "x0_nan":        # every row
        x0[col] = np.nan
    elif kind == "neg_zero":
        # row 0: every difference +0.0 or -0.0 (distance +0.0); row B // 2:
        # -0.0 - 0.0 in one column; every row: a -0.0 weight in the next one
        x[0] = x0
        x0[col] = 0.0
        x[0, col] = -0.0
        x[B // 2, col] = -0.0
        wf[(col + 1) % S] = -0.0 if S > 1 else wf[0]
    else:
        raise ValueError(kind)
    return x, x0, wf
