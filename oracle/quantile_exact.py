"""Exact weighted-quantile reference, and the inputs that aim the device
select (abc_quantile.hip) and its sort-based fallback at their edges.

Test infrastructure only -- see ``oracle/__init__.py``.

``oracle.weighted_quantile`` is float64: its ``cumsum`` rounds N times, and
between two clusters of points the interpolation slope multiplies that
rounding by ~N (half the points near 1, half near 1000, N = 2^20 + 1: the
float64 oracle is 1.3e-9 relative away from an 80-bit cumsum).  Two things
here take the rounding out of the comparison:

* ``dyadic_weights`` -- integer weights m_i whose sum is a power of two
  below 2^53, taken as w = m / 2^k.  Every partial sum of such weights, in
  any order, is exact in float64, the total is exactly 1.0 and cs - w / 2 is
  exact.  A sequential cumsum, a tree sum and a fixed-point search then see
  the same numbers, and the only freedom left in the quantile is the final
  ``slope * (alpha - xj) + yj``.
* ``ExactQuantile`` -- the stable order, the cumulative sums in Python-exact
  integers (dyadic input) or ``np.longdouble`` (general input), and
  np.interp's rules restated on them.
"""
import collections
import zlib

import numpy as np

LD = np.longdouble

KINDS = ("flat", "skew", "dominant", "zeros", "edge_zeros", "staircase")


def seed(name):
    """One generator per case name (the device tests and the host tests of
    the reference build the same inputs from it)."""
    return np.random.default_rng(zlib.crc32(name.encode()))


def dyadic_weights(rng, N, kind, points=None, heavy=None):
    """Integer weights m (int64) with sum m = 2^k < 2^53 -> (w, m, k) with
    w = m / 2^k (float64, exact).  The kinds below are scaled up to the power
    of two; the sum is fixed up on the largest entry.

    flat        m uniform in [1, 2^20)
    skew        max(1, floor(256 exp(3 z)))
    dominant    all 1, one entry 2^40 (at index ``heavy``; default: the point
                of median rank in the stable order of ``points``)
    zeros       flat with 40 % of the entries 0
    edge_zeros  flat with the weights of the 50 smallest and the 50 largest
                ``points`` 0
    staircase   19 on the lower half of ``points``, 40960 on the upper half,
                10 * 2^(62 - ceil log2 N) on the largest (see below)
    """
    if kind in ("flat", "zeros", "edge_zeros"):
        m = rng.integers(1, 1 << 20, N, dtype=np.int64)
        if kind == "zeros":
            m[rng.uniform(size=N) < 0.4] = 0
            if not m.any():
                m[0] = 1
        elif kind == "edge_zeros":
            assert points is not None and N > 100
            order = np.argsort(points, kind="stable")
            m[order[:50]] = 0
            m[order[-50:]] = 0
    elif kind == "skew":
        m = np.maximum(1, np.floor(256.0 * np.exp(3.0 * rng.standard_normal(N)))
                       ).astype(np.int64)
    elif kind == "dominant":
        m = np.ones(N, dtype=np.int64)
        if heavy is None:
            heavy = (int(np.argsort(points, kind="stable")[N // 2])
                     if points is not None else N // 2)
        m[heavy] = 1 << 40
    elif kind == "staircase":
        # the select's fixed-point weights are w * 2^(62 - ceil log2 N) / max w,
        # truncated.  The lower half of the points gets ~1.9 units each (0.9
        # lost per point, ~N / 2 units in all), the upper half 4096 units
        # (nothing lost), the largest point the maximum.  At a knot in the
        # upper half the truncated cumulative weight is short of alpha x total
        # by ~0.45 N units = N / 9000 of those points: more than the one bin
        # of slack next to the target bin, less than the pick's margin.
        assert points is not None and N > 16
        order = np.argsort(points, kind="stable")
        m = np.empty(N, dtype=np.int64)
        m[order[:N // 2]] = 19
        m[order[N // 2:]] = 40960
        m[order[-1]] = 10 << (62 - max(0, (N - 1).bit_length()))
    else:
        raise ValueError(kind)
    # up to the next power of two: every entry grows in proportion (a factor
    # below 2: the kind keeps its shape -- all of the missing weight on one
    # entry would make every kind a dominant one, up to half the mass on one
    # point), and what the floors leave over goes to the largest entry
    s = int(m.sum())
    k = max(0, (s - 1).bit_length())
    m += np.floor(m * (((1 << k) - s) / s)).astype(np.int64)
    m[int(np.argmax(m))] += (1 << k) - int(m.sum())
    assert int(m.sum()) == 1 << k and k < 53 and m.min() >= 0
    return np.ldexp(m.astype(np.float64), -k), m, k


POINT_RECIPES = ("normal", "heavy_ties", "one_value", "two_spikes", "dense_core",
                 "crowded", "discrete", "symmetric", "wide", "subnormal", "zeros_pm",
                 "outliers", "inf30", "two_cluster")


def points_recipe(rng, N, recipe):
    """The data shapes of the device tests (float64 [N])."""
    if recipe == "normal":              # continuous, positive
        return rng.gamma(2.0, 1.5, N)
    if recipe == "heavy_ties":          # 30 % of the points on one value
        pts = rng.gamma(2.0, 1.5, N)
        pts[rng.uniform(size=N) < 0.3] = 2.5
        return pts
    if recipe == "one_value":
        return np.full(N, 1.25)
    if recipe == "two_spikes":          # two adjacent doubles
        return np.where(rng.uniform(size=N) < 0.5, 1.0, np.nextafter(1.0, 2.0))
    if recipe == "dense_core":          # half the points in 1e-4 of the range
        return np.where(rng.uniform(size=N) < 0.5, 1.0 + rng.uniform(size=N),
                        1.5 + 1e-4 * rng.uniform(size=N))
    if recipe == "crowded":             # the bulk next to two extreme points
        pts = 1.0 + 1e-3 * rng.uniform(size=N)
        pts[7], pts[N // 2] = 1e-300, 1e300
        return pts
    if recipe == "discrete":            # integer-valued distances
        return rng.integers(0, 40, N).astype(np.float64)
    if recipe == "symmetric":           # the span crosses the keys' sign fold
        return rng.standard_normal(N)
    if recipe == "wide":                # most of the 64 key bits
        sign = np.where(rng.uniform(size=N) < 0.5, -1.0, 1.0)
        return sign * np.exp(20.0 * rng.standard_normal(N))
    if recipe == "subnormal":           # k * 5e-324, both zeros among them
        k = rng.integers(-1000, 1001, N)
        pts = k * 5e-324
        pts[(k == 0) & (rng.uniform(size=N) < 0.5)] = -0.0
        return pts
    if recipe == "zeros_pm":            # one key: ties by index
        return np.where(rng.uniform(size=N) < 0.5, -0.0, 0.0)
    if recipe == "outliers":            # one value between two lone extremes
        pts = np.ones(N)
        pts[7], pts[N // 2] = -1e300, 1e300
        return pts
    if recipe == "inf30":               # failed simulations: 30 % at +inf
        pts = rng.gamma(2.0, 1.5, N)
        pts[rng.uniform(size=N) < 0.3] = np.inf
        return pts
    if recipe == "two_cluster":         # half near 1, half near 1000
        return np.where(rng.uniform(size=N) < 0.5, 1.0 + 1e-3 * rng.uniform(size=N),
                        1000.0 + rng.uniform(size=N))
    raise ValueError(recipe)


Result = collections.namedtuple("Result", "q xj xj1 yj yj1 clamp copy j")
Result.__doc__ = """q (float64-rounded), the bracketing knots (xp as
np.longdouble, y as float64), clamp: alpha lay outside [xp_0, xp_{N-1}];
copy: q is a copy of one input point (a clamp, an exact knot hit, or the
last knot); j: the left knot's rank (-1 / N at the clamps)."""


class ExactQuantile:
    """weighted_quantile(points, w, alpha) without float64 summation error.

    xp = (cs - w / 2) / cs[-1] over the stable order of the points, as both
    device kernels compute it.  (The reference function,
    pyabc/weighted_statistics.py:27-43, omits the division: its caller,
    QuantileEpsilon._update, normalises the weights beforehand.)  ``w`` of an
    integer dtype is summed exactly (int64; the caller keeps the total below
    2^62) and the knots are exact whenever 2 * total fits the longdouble's 64
    mantissa bits' ratio -- in particular for ``dyadic_weights``; a float
    ``w`` is cumulated in np.longdouble.  Negative and non-finite weights
    count as 0, as in the kernels.

    np.interp's rules (numpy compiled_base.c, arr_interp), restated:
      alpha > xp[N-1] -> fp[N-1];  alpha < xp[0] -> fp[0];
      j = #(xp <= alpha) - 1;  j == N - 1 -> fp[j];  xp[j] == alpha -> fp[j];
      else slope = (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]),
           r = slope * (alpha - xp[j]) + fp[j];
           r NaN -> r = slope * (alpha - xp[j+1]) + fp[j+1];
           still NaN and fp[j] == fp[j+1] -> fp[j]        (inf - inf)
    evaluated in np.longdouble and rounded once.  A total weight that is not
    positive leaves no knots: q = NaN.
    """

    def __init__(self, points, w):
        p = np.asarray(points, dtype=np.float64)
        self.order = np.argsort(p, kind="stable")
        self.p = p[self.order]
        w = np.asarray(w)
        if np.issubdtype(w.dtype, np.integer):
            m = w[self.order].astype(np.int64)
            cs = np.cumsum(m)
            self.total = LD(int(cs[-1]))
            num = (2 * cs - m).astype(LD)       # < 2^63: exact
            self.xp = num / (2 * self.total) if cs[-1] > 0 else None
        else:
            wl = np.asarray(w, dtype=np.float64)[self.order]
            wl = np.where((wl > 0) & np.isfinite(wl), wl, 0.0).astype(LD)
            cs = np.cumsum(wl)
            self.total = cs[-1]
            self.xp = (cs - wl / 2) / cs[-1] if cs[-1] > 0 else None
        self.N = len(self.p)

    def knot(self, j):
        """xp_j as a float64 (exact for dyadic weights)."""
        return float(self.xp[j])

    def __call__(self, alpha):
        p, xp, n = self.p, self.xp, self.N
        nan = float("nan")
        if xp is None:
            return Result(nan, LD(nan), LD(nan), nan, nan, False, False, -1)
        a = LD(alpha)
        if a > xp[-1]:
            return Result(float(p[-1]), xp[-1], xp[-1], p[-1], p[-1], True, True, n)
        if a < xp[0]:
            return Result(float(p[0]), xp[0], xp[0], p[0], p[0], True, True, -1)
        j = int(np.searchsorted(xp, a, side="right")) - 1
        if j == n - 1:
            return Result(float(p[j]), xp[j], xp[j], p[j], p[j], False, True, j)
        xj, xj1, yj, yj1 = xp[j], xp[j + 1], p[j], p[j + 1]
        if xj == a:
            return Result(float(yj), xj, xj1, yj, yj1, False, True, j)
        with np.errstate(invalid="ignore", over="ignore"):
            slope = (LD(yj1) - LD(yj)) / (xj1 - xj)
            r = slope * (a - xj) + LD(yj)
            if np.isnan(r):
                r = slope * (a - xj1) + LD(yj1)
                if np.isnan(r) and yj == yj1:
                    r = LD(yj)
        return Result(float(r), xj, xj1, yj, yj1, False, False, j)


def weighted_quantile_exact(points, w, alpha):
    """One quantile -> ``Result`` (see ``ExactQuantile``, which keeps the
    order and the knots for several alphas)."""
    return ExactQuantile(points, w)(alpha)


# ---- the tolerance model (stated in tests/test_gpu_quantile.py) ---------------

EPS = float(np.finfo(np.float64).eps)


def ulp_max(res):
    """ulp(max(|y_j|, |y_j1|)) of a result with finite knots."""
    return float(np.spacing(max(abs(res.yj), abs(res.yj1))))


def budget_dyadic(res):
    """Dyadic weights and finite knots: 4 ulp of the larger knot value; 0
    where q is a copy of an input point or not finite."""
    if res.copy or not np.isfinite(res.q) or not np.isfinite(res.yj1 - res.yj):
        return 0.0
    return 4.0 * ulp_max(res)


def budget_general(res, N):
    """(whole budget, its summation part): 1e-12 |q| + N eps |dy| / dxp --
    the worst-case rounding of a sum of N non-negative terms, pushed through
    the interpolation slope."""
    if not np.isfinite(res.q):
        return 0.0, 0.0
    dy = abs(float(res.yj1) - float(res.yj))
    dx = float(res.xj1 - res.xj)
    part = N * EPS * dy / dx if dy > 0 and dx > 0 else 0.0
    return 1e-12 * abs(res.q) + part, part


def same_value(q, ref):
    """Equal as numbers (-0.0 == +0.0: the kernels' keys fold the two), or
    both NaN."""
    return (q == ref) or (q != q and ref != ref)


def alpha_set(ref, exact_knots=True, extra=()):
    """The alphas of the device tests: 0 and 1; below xp_0 and above
    xp_{N-1} where there is room; the knots j = N // 3, 0 and N - 1 (exact
    with dyadic weights) and the midpoints next to them; 0.1, 0.5, 0.9."""
    n = ref.N
    out = [0.0, 1.0, 0.1, 0.5, 0.9]
    x0, xn = float(ref.xp[0]), float(ref.xp[-1])
    if x0 > 0:
        out.append(x0 / 2)
    if xn < 1:
        out.append(xn + (1 - xn) / 2)
    for j in sorted({n // 3, 0, n - 1}):
        xj = float(ref.xp[j])
        if exact_knots:
            out.append(xj)
        if j + 1 < n:
            out.append(xj + (float(ref.xp[j + 1]) - xj) / 2)
        if j > 0:
            out.append(xj - (xj - float(ref.xp[j - 1])) / 2)
    out.extend(extra)
    return [a for a in dict.fromkeys(out) if 0.0 <= a <= 1.0]


# ---- the cases both test files build --------------------------------------------
# case -> (points recipe, dyadic weight kind)
SHAPE_CASES = {            # the data shapes of test_weighted_quantile_select
    "normal": ("normal", "flat"), "skewed_w": ("normal", "skew"),
    "heavy_ties": ("heavy_ties", "flat"), "one_value": ("one_value", "flat"),
    "two_spikes": ("two_spikes", "flat"), "zero_w": ("normal", "zeros"),
    "dense_core": ("dense_core", "flat"), "crowded": ("crowded", "flat"),
    "discrete": ("discrete", "flat")}
# the select itself must decide these (no knot inside ties by the thousand)
SHAPE_DECIDED = ("normal", "skewed_w", "zero_w", "dense_core")
KEY_CASES = {k: (k, "flat") for k in ("symmetric", "wide", "subnormal", "zeros_pm",
                                      "outliers", "inf30")}
WEIGHT_CASES = {"dominant": ("normal", "dominant"), "edge_zeros": ("normal", "edge_zeros"),
                "staircase": ("normal", "staircase")}
GENERAL_CASES = {          # case -> (points recipe, general weight kind)
    "uniform": ("normal", "uniform"), "exp6": ("normal", "exp6"),
    "two_cluster_uniform": ("two_cluster", "uniform"),
    "two_cluster_exp6": ("two_cluster", "exp6")}


def dyadic_case(case, N):
    """-> (points, w, m) of a SHAPE / KEY / WEIGHT case at N points."""
    recipe, kind = {**SHAPE_CASES, **KEY_CASES, **WEIGHT_CASES}[case]
    rng = seed(f"{case}:{N}")
    pts = points_recipe(rng, N, recipe)
    w, m, _ = dyadic_weights(rng, N, kind, points=pts)
    return pts, w, m


def general_case(case, N):
    """-> (points, w): float weights normalised by numpy's float64 sum."""
    recipe, kind = GENERAL_CASES[case]
    rng = seed(f"{case}:{N}")
    pts = points_recipe(rng, N, recipe)
    w = (rng.uniform(0.5, 1.5, N) if kind == "uniform"
         else np.exp(6.0 * rng.standard_normal(N)))
    return pts, w / w.sum()


def inf_alphas(ref):
    """inf30's extra alphas: inside the inf run, and the last finite knot,
    the first inf knot and their midpoint."""
    f = int(np.searchsorted(ref.p, np.inf, side="left"))   # first inf rank
    a, b = ref.knot(f - 1), ref.knot(f)
    return [ref.knot(f + (ref.N - f) // 2), a, b, a + (b - a) / 2]


def dominant_alphas(ref, m):
    """Just below, at and just above the heavy point's knot, and 0.5."""
    h = int(np.nonzero(ref.order == int(np.argmax(m)))[0][0])
    x = ref.knot(h)
    return [float(np.nextafter(x, 0.0)), x, float(np.nextafter(x, 1.0)), 0.5]


def staircase_alphas(ref):
    """Knots in the upper half of a staircase input, and the midpoints next
    to them."""
    n, out = ref.N, []
    for j in (n // 2 + n // 8, n // 2 + n // 4, n - 3):
        out += [ref.knot(j), (ref.knot(j) + ref.knot(j + 1)) / 2]
    return out
