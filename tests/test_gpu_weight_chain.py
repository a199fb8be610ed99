"""The weight chain against exact references (oracle/weights_exact.py):

    abc_importance_weights -> abc_normalize_weights (+ ESS)
    -> abc_weighted_moments -> abc_inclusive_scan_f64
    -> the ancestor searches (plain, cdf guide, ancestor table).

float64 numpy is a peer of these kernels and cannot measure them; the
references here are exact integers (sums, ESS, moments, cdf) or mpmath (exp),
rounded once.  Every bound below is derived from the kernels' code -- the
number of roundings a term can meet -- and stated next to its test; none is
fitted to a kernel's output.  u = 2^-53 (unit roundoff), eps = 2 u.  Each test
prints ``CHAIN <what> K=<derived> measured=<largest, same units>``.

How far float64 numpy itself sits from the exact values on the same inputs
(the reference alone, for context).  np.cov(X, aweights=w) x (1 - sum w^2 /
(sum w)^2) at N = 257, d = 3, in units of eps A_ab + eps^2 M_a M_b: 3.3
(ratio1), 3.6 (ratio1e6), 5.0 (ratio1e10: 1.4e5 eps A, the rest is its mean's
error squared), 2.8 (scales), 11 (constant), 1.6 (rank_deficient), 3.8
(zero_weights); on `dominant` the conversion from the unbiased estimate
cancels 12 digits and says nothing about np.cov.  np.cumsum at N = 524289 is
sequential, hence nondecreasing, and 19 (ascending) to 2.9e3 (descending)
eps x total away from the exact cdf -- the kernel's bound there is 260.5.
"""
import math

import numpy as np
import pytest

from oracle import weights_exact as wx
from oracle.philox import philox4x32_10, uniform53

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS, U, TINY = wx.EPS, wx.U, wx.TINY
DBL_MAX = float(np.finfo(np.float64).max)
DBL_MIN = float(np.finfo(np.float64).tiny)


@pytest.fixture(scope="module")
def dev():
    from pyabc_amd import gpu
    return gpu.require_device()


def T(a, dtype=None):
    from pyabc_amd import gpu
    return gpu.as_dev(a, dtype=dtype)


def report(what, K, measured):
    print(f"CHAIN {what} K={K:.6g} measured={measured:.6g}")


_cache = {}


def cached(key, fn):
    """Oracle results, once per module."""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def ceil_div(a, b):
    return -(-a // b)


# ---- importance weights -------------------------------------------------------

IW_EDGES = [-760.0, -745.2, -744.0, -710.0, -708.3, -700.5, -700.0, -0.0, 0.0,
            700.0, 700.5, 709.7, 709.9, 710.5, 711.0, 720.0]


def iw_inputs(A):
    rng = np.random.default_rng(1000 + A)
    x = rng.uniform(-760.0, 720.0, A)
    if A >= len(IW_EDGES):
        x[:len(IW_EDGES)] = IW_EDGES
    lt = rng.uniform(-300.0, 300.0, A)
    lp = x + lt
    if A >= 255:      # IEEE specials, away from the edge values
        lp[100], lt[101], lp[102], lt[103] = -np.inf, -np.inf, np.nan, np.nan
        lp[104] = lt[104] = -np.inf
    accw = rng.uniform(0.5, 2.0, A)
    return lp, lt, accw


@pytest.mark.parametrize("with_accw", [False, True])
@pytest.mark.parametrize("A", [0, 1, 255, 256, 257, 4099])
def test_importance_weights(dev, A, with_accw):
    """w = exp(lp - lt) * scale [* acc_w], scale = 0.3, lp - lt over
    [-760, 720]: results from 0 through the subnormals up to overflow.

    The kernel rounds x = lp - lt (relative u, so exp(x) moves by |x| u),
    takes the device exp and multiplies left to right.  The device library
    documents exp(double) at 1 ulp (OCML's accuracy table; the HIP math API
    table says the same), and a correctly rounded multiply is 1/2 ulp, counted
    here as 1 ulp per multiply.  1 ulp <= eps relative:

        |x| <= 700:  |x| eps / 2 + 1 eps (exp) + (1 + acc) eps (multiplies)
        |x| >  700:  exp(x) is taken as exp(x / 2)^2 around the other factors
                     (x / 2 is exact): exp's ulp counts twice and there is one
                     multiply more: |x| eps / 2 + 2 eps + (2 + acc) eps
        + eps / 2 for the reference's own rounding.

    A subnormal (intermediate or final) result is instead good to one
    subnormal spacing (2^-1074) per operation -- exp and each multiply --
    scaled by the factors > 1 that may follow: (2 + acc + 1) 2^-1074 x
    max(1, scale) max(1, acc_w).  Where the exact value is within the relative
    bound of the largest double, inf and a finite value are both accepted.
    lp = -inf -> exactly 0; lt = -inf -> +inf; NaN -> NaN."""
    from pyabc_amd import gpu
    scale = 0.3
    lp, lt, accw = iw_inputs(A)
    aw = accw if with_accw else None
    got = gpu.importance_weights(T(lp), T(lt), scale,
                                 T(aw) if with_accw else None).cpu().numpy()
    assert got.shape == (A,)
    if A == 0:
        return
    ref = cached(("iw", A, with_accw),
                 lambda: wx.importance_weight_exact(lp, lt, scale, aw))
    with np.errstate(invalid="ignore"):
        x = np.abs(lp - lt)
    acc = 1 if with_accw else 0
    split = x > 700.0
    rel = x * EPS / 2 + np.where(split, 2, 1) * EPS \
        + np.where(split, 2 + acc, 1 + acc) * EPS + EPS / 2
    absb = (3 + acc) * TINY * max(1.0, scale) * (np.maximum(1.0, accw) if with_accw else 1.0)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    if A >= 255:
        assert got[100] == 0.0 and got[101] == np.inf and nan[102:105].all()
        # the inputs do cross both edges
        fin = ref[np.isfinite(ref)]
        assert (fin == 0).any() and ((fin > 0) & (fin < DBL_MIN)).any()
        assert (ref == np.inf).any() and (fin > 1e300).any()
    worst = 0.0
    for i in np.nonzero(~nan)[0]:
        g, r = got[i], ref[i]
        if not math.isfinite(x[i]):          # lp or lt infinite: 0 or inf, exactly
            assert g == r, (i, g, r)
            continue
        if math.isinf(r) or math.isinf(g):
            near = (DBL_MAX * (1 - rel[i]) <= (g if math.isinf(r) else r))
            assert (g == r) or near, (i, lp[i] - lt[i], g, r)
            continue
        tol = rel[i] * r + (absb[i] if with_accw else absb)
        err = abs(g - r)
        assert err <= tol, (i, lp[i] - lt[i], g, r, err / tol)
        worst = max(worst, err / tol)
    report(f"importance A={A} acc={acc}", 1.0, worst)


# ---- normalise / ESS --------------------------------------------------------------

NW_N = [1, 2, 255, 256, 257, 65536, 65537]
NW_K = [-1000, -600, -520, 0, 500, 520]
NW_FAMILIES = ["exponential", "dominant", "decades", "half_zeros", "equal"]


def nw_family(family, N):
    rng = np.random.default_rng(2000 + N)
    if family == "exponential":
        return rng.exponential(size=N)
    if family == "dominant":             # ESS -> 1
        w = rng.uniform(0.5, 1.5, N)
        w[N // 2] = 1e12
        return w
    if family == "decades":
        return 10.0 ** rng.uniform(-300.0, 0.0, N)
    if family == "half_zeros":
        w = rng.uniform(0.5, 1.5, N)
        w[rng.uniform(size=N) < 0.5] = 0.0
        w[N // 2] = 1.25
        return w
    if family == "equal":                # 3 significant bits: k * w is exact
        return np.full(N, 0.375)
    raise ValueError(family)


def nw_depth(N):
    """Roundings a term of sum w can meet (wsum_kernel / wsum_final): the
    thread's grid-stride adds, 6 butterfly levels, 3 adds over the waves, one
    add per block in the final."""
    nblk = min(ceil_div(N, 256), 256)
    return ceil_div(N, nblk * 256) + 6 + 3 + nblk


def _normalize(w):
    from pyabc_amd import gpu
    wd = T(w)
    stats = gpu.normalize_weights(wd)
    return wd.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("N", NW_N)
@pytest.mark.parametrize("family", NW_FAMILIES)
def test_normalize_and_ess_at_every_scale(dev, family, N):
    """w / sum w and the ESS against the exact values, for the family times
    2^k, k in NW_K.  Where 2^k w is exact (every entry still a normal double;
    the 300-decade family underflows for k < 0 and is then measured against
    the exact values of what the device was given) the exact ESS and
    normalised weights are those of k = 0, and the device returns the SAME
    BITS as at k = 0: every partial sum scales exactly.

    With D = nw_depth(N) roundings on sum w:
        |sum - exact|  <= (D + 1) u exact            (+1: the reference's)
        |w_n - exact|  <= (D + 2) u exact + 2^-1074  (the division)
        |ESS - exact|  <= (3 D + 5) u exact: ESS = 1 / sum w_n^2; a square
            carries 2 (D + 1) u + u, the sum D u more, the reciprocal and the
            reference u each.  Squares below 2^-1022 lose bits, but against a
            sum >= 1 / N that is N^2 2^-1075.
    sum w^2 of the raw weights is only compared where it is a normal double.
    N = 1: w = 1.0 and ESS = 1.0 exactly; equal weights at N a power of two:
    ESS = N exactly."""
    base_w = nw_family(family, N)
    D = nw_depth(N)
    first = None
    worst = dict(sum=0.0, wn=0.0, ess=0.0)
    for k in NW_K:
        w = np.ldexp(base_w, k)
        exact_scaling = bool(np.array_equal(np.ldexp(w, -k), base_w)
                             and (w[w > 0] >= DBL_MIN).all())
        ref = cached(("nw", family, N, 0 if exact_scaling else k),
                     lambda: wx.exact_sums(base_w if exact_scaling else w))
        wn, st = _normalize(w)
        what = (family, N, k)
        if not w.any():          # every weight underflowed: the all-zero case
            assert st[0] == 0.0 and math.isnan(st[1]) and np.isnan(wn).all(), what
            continue
        ref_sum = math.ldexp(ref.sum, k) if exact_scaling else ref.sum
        assert abs(st[0] - ref_sum) <= (D + 1) * U * ref_sum, what
        worst["sum"] = max(worst["sum"], abs(st[0] - ref_sum) / (U * ref_sum))
        err = np.abs(wn - ref.normalised)
        tol = (D + 2) * U * ref.normalised + TINY
        assert (err <= tol).all(), (what, np.max(err / tol))
        assert ((wn == 0) == (w == 0)).all() or family == "decades", what
        worst["wn"] = max(worst["wn"], float(np.max(err / (U * ref.normalised + TINY))))
        assert abs(st[1] - ref.ess) <= (3 * D + 5) * U * ref.ess, (what, st[1], ref.ess)
        worst["ess"] = max(worst["ess"], abs(st[1] - ref.ess) / (U * ref.ess))
        with np.errstate(over="ignore", under="ignore"):
            ref_s2 = float(np.ldexp(ref.sum_sq, 2 * k)) if exact_scaling else ref.sum_sq
        if DBL_MIN * 2.0 ** 60 <= ref_s2 < math.inf:
            assert abs(st[2] - ref_s2) <= (D + 2) * U * ref_s2, what
        if exact_scaling:
            if first is None:
                first = (wn, st[1])
            assert np.array_equal(wn, first[0]) and st[1] == first[1], what
        if N == 1:
            assert wn[0] == 1.0 and st[1] == 1.0, what
        if family == "equal" and N & (N - 1) == 0:
            assert st[1] == float(N) and (wn == 1.0 / N).all(), what
    assert first is not None
    report(f"normalize sum {family} N={N}", D + 1, worst["sum"])
    report(f"normalize w_n {family} N={N}", D + 2, worst["wn"])
    report(f"normalize ESS {family} N={N}", 3 * D + 5, worst["ess"])


@pytest.mark.parametrize("N", [1, 257, 65537])
def test_normalize_all_zero_weights(dev, N):
    """Pinned (include/abcgpu.h): sum 0, sum w^2 0, every weight and the ESS
    NaN; no error."""
    wn, st = _normalize(np.zeros(N))
    assert st[0] == 0.0 and st[2] == 0.0 and math.isnan(st[1])
    assert np.isnan(wn).all()


def test_population_ess_does_not_depend_on_the_weight_scale(dev):
    """Through Population.from_columns and the ESS accessors of smc.py: raw
    importance weights at scale 2^-600 (a tight kernel in many dimensions)
    and at scale 1 are the same population."""
    from pyabc_amd.population import ColumnarParticles, Population
    from pyabc_amd.smc import ABCSMC
    rng = np.random.default_rng(7)
    N = 1000
    w = rng.exponential(size=N) + 0.01
    theta = T(rng.standard_normal((N, 2)))
    out = []
    for k in (0, -600):
        cols = ColumnarParticles(theta, T(np.ldexp(w, k)), T(rng.uniform(size=N)),
                                 None, ["a", "b"], [])
        pop = Population.from_columns(cols)
        out.append((ABCSMC._ess(pop), ABCSMC._ess_async(pop)(),
                    cols.weights.cpu().numpy()))
    ref = wx.exact_sums(w)
    assert out[0][0] == out[1][0] == out[0][1] == out[1][1]
    assert np.array_equal(out[0][2], out[1][2])
    assert abs(out[0][0] - ref.ess) <= (3 * nw_depth(N) + 5) * U * ref.ess


# ---- moments ---------------------------------------------------------------------

MOM_FAST = [1, 2, 3, 4, 5, 6, 8, 10, 12, 16]
MOM_GENERIC = [7, 33, 64]          # 64: all 16 x 256 pair slots of the LDS path
MOM_WIDE = [65, 130]
MOM_N = [1, 2, 63, 64, 65, 255, 256, 257, 4097]
MOM_POPS = ["ratio1", "ratio1e6", "ratio1e10", "scales", "dominant", "constant",
            "rank_deficient", "zero_weights"]


def mom_depth(N, d):
    """Additions a term of one of the kernels' sums can meet, per path
    (abc_reduce.hip)."""
    if d in MOM_FAST:      # thread's strided rows, butterfly 6, 2 LDS levels,
        nblk = min(ceil_div(N, 256), 256)          # then per lane + butterfly 6
        return ceil_div(N, nblk * 256) + 6 + 2 + ceil_div(nblk, 64) + 6
    if d <= 64:            # 64 staged rows, one add per stage, one per block
        nblk = min(ceil_div(N, 64), 256)
        return 64 + ceil_div(ceil_div(N, 64), nblk) + nblk
    nb = max(1, min(N, min((1 << 24) // (d * d), 256)))   # rows strided by nb
    return ceil_div(N, nb) + nb


def mom_K(N, d):
    """In eps.  With D = mom_depth: a term w x of the mean meets 1 product
    rounding and D additions, sum w D additions, then one division (two on
    the fast path, which divides once for the centring and once for the
    output; the same quotient): Km = (2 D + 3) / 2.  A term w (x_a - m_a)(x_b - m_b) meets 2 subtractions,
    2 products, D additions and the division by sum w (D more): Kc =
    (2 D + 5) / 2 -- at most: a fused multiply-add only removes roundings.
    The computed mean is off by dm, |dm_a| <= Km eps M_a, and the centred sums
    see it at second order: dm_a dm_b exactly (the first-order terms cancel
    as sum w (x - m) = 0) plus the roundings made on it, Kc eps (|dm_a| B_b +
    |dm_b| B_a) with B = sum w |x - m| / sum w <= 2 M.  One K = Km + 2 Kc
    covers all three: K >= Kc, K >= Km and K^2 >= Km^2 + 4 Km Kc."""
    D = mom_depth(N, d)
    return (2 * D + 3) / 2 + (2 * D + 5)


def mom_population(pop, N, d):
    rng = np.random.default_rng(3000 + 131 * N + d)
    X = rng.standard_normal((N, d))
    w = rng.uniform(0.05, 1.0, N)
    if pop == "ratio1":
        X += 1.0
    elif pop == "ratio1e6":
        X += 1e6
    elif pop == "ratio1e10":
        X += 1e10
    elif pop == "scales":
        X = (X + 0.5) * 10.0 ** np.linspace(-100.0, 100.0, d)
    elif pop == "dominant":             # one weight holds 1 - 1e-12 of the mass
        h = N // 2
        w[h] = 0.0
        w[h] = max(w.sum(), 1.0) * 1e12
    elif pop == "constant":
        X[:, 0] = 0.1
        if d > 2:
            X[:, d - 1] = -1e5
    elif pop == "rank_deficient":       # rank 1 scatter about an offset
        X = np.outer(rng.standard_normal(N), rng.standard_normal(d)) + 3.0
    elif pop == "zero_weights":         # finite rows that must not count
        z = np.arange(N) % 3 == 1
        w[z] = 0.0
        X[z] = 1e150
        if not w.any():
            w[0] = 0.5
    else:
        raise ValueError(pop)
    return X, w


def mom_cases():
    out = []
    for d in MOM_FAST + MOM_GENERIC + MOM_WIDE:
        ns = [n for n in MOM_N if d < 64 or n <= 257]
        out += [(d, n, "ratio1") for n in ns]
        out += [(d, 257, pop) for pop in MOM_POPS[1:]]
        if d in (1, 3, 7):   # MOM_ROWS * MOM_BLOCKS + 1, 256 * 256 + 1
            out += [(d, n, pop) for n in (16385, 65537) for pop in ("ratio1", "ratio1e6")]
    return out


def _moments(X, w):
    from pyabc_amd import gpu
    return gpu.weighted_moments(T(X), T(w), with_max=True)


@pytest.mark.parametrize("d,N,pop", mom_cases())
def test_weighted_moments_exact(dev, d, N, pop):
    """Every dispatch path (fast: d in MOM_FAST; generic LDS: 7, 33, 64; wide:
    65, 130), block boundaries in N, and populations two-pass centring must
    survive, against exact integer moments:

        max w             equal
        |d sum w|         <= (D + 1) u sum w;  |d sum w^2| <= (D + 2) u sum w^2
        |d mean_a|        <= K eps M_a
        |d cov_ab|        <= K eps A_ab + (K eps)^2 M_a M_b
    A_ab = sum w |x_a-m_a| |x_b-m_b| / sum w, M_a = sum w |x_a| / sum w,
    D = mom_depth, K = mom_K (derived there; D = 20, K = 66.5 on the fast path
    at N = 65537, D = 325, K = 981.5 on the LDS path, D = 258, K = 780.5 on
    the wide path at N = 257).  The reference rounds once more: + u on each."""
    X, w = mom_population(pop, N, d)
    ref = cached(("mom", d, N, pop), lambda: wx.exact_moments(X, w))
    sw, sw2, mean, cov, wmax = _moments(X, w)
    D, K = mom_depth(N, d), mom_K(N, d)
    own = ref.own_error + U
    assert wmax == ref.max
    assert abs(sw - ref.sum) <= (D + 1) * U * ref.sum
    assert abs(sw2 - ref.sum_sq) <= (D + 2) * U * ref.sum_sq
    tol_m = (K * EPS + own) * ref.M
    em = np.abs(mean - ref.mean)
    assert (em <= tol_m).all(), (em / tol_m).max()
    tol_c = (K * EPS + own) * ref.A + (K * EPS) ** 2 * np.outer(ref.M, ref.M)
    ec = np.abs(cov - ref.cov)
    assert (ec <= tol_c).all(), (ec / tol_c).max()
    # bitwise reproducible run to run
    again = _moments(X, w)
    assert np.array_equal(again[3], cov) and np.array_equal(again[2], mean)
    assert again[0] == sw and again[1] == sw2
    unit_m = EPS * ref.M
    unit_c = EPS * ref.A + K * EPS ** 2 * np.outer(ref.M, ref.M)
    with np.errstate(invalid="ignore", divide="ignore"):
        report(f"moments d={d} N={N} {pop}", K,
               max(np.nanmax(np.where(unit_m > 0, em / unit_m, 0.0)),
                   np.nanmax(np.where(unit_c > 0, ec / unit_c, 0.0))))


@pytest.mark.parametrize("d", [3, 7, 65])
@pytest.mark.parametrize("k", [400, -400])
def test_weighted_moments_weight_scale(dev, d, k):
    """w -> 2^k w is exact in every product and sum: sum w scales by exactly
    2^k, sum w^2 by 2^2k, max w by 2^k, and the mean and the covariance keep
    their bits."""
    X, w = mom_population("ratio1e6", 257, d)
    a = _moments(X, w)
    b = _moments(X, np.ldexp(w, k))
    assert b[0] == math.ldexp(a[0], k) and b[1] == math.ldexp(a[1], 2 * k)
    assert b[4] == math.ldexp(a[4], k)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


# ---- scan ---------------------------------------------------------------------------

SCAN_N = [1, 7, 8, 9, 2047, 2048, 2049, 524289]   # 524289: 257 tiles
SCAN_FAMILIES = ["uniform", "zeros70", "decades", "exp40", "dominant",
                 "ascending", "descending"]


def scan_family(family, N, seed=0):
    rng = np.random.default_rng(4000 + N + seed)
    if family == "uniform":
        return rng.uniform(size=N)
    if family == "zeros70":        # leading and trailing runs of zeros too
        w = rng.uniform(size=N)
        w[rng.uniform(size=N) < 0.7] = 0.0
        if N > 12:
            w[:5] = 0.0
            w[-5:] = 0.0
        w[N // 2] = 0.625
        return w
    if family == "decades":
        return 10.0 ** rng.uniform(-300.0, 0.0, N)
    if family == "exp40":
        return np.exp(-40.0 * rng.uniform(size=N))
    if family == "dominant":       # one heavy row in the middle
        w = rng.uniform(size=N)
        w[N // 2] = 1e12
        return w
    if family == "ascending":
        return np.sort(np.exp(-40.0 * rng.uniform(size=N)))
    if family == "descending":
        return np.sort(np.exp(-40.0 * rng.uniform(size=N)))[::-1].copy()
    raise ValueError(family)


def scan_roundings(N):
    """Roundings a term can meet in abc_inclusive_scan_f64: the thread's 8
    items in order, the 256 thread sums of the tile in order, the tile sums in
    order (the two joining additions are counted in the 8 and the 256, whose
    chains have one addition fewer than terms)."""
    return 8 + 256 + ceil_div(N, 2048)


def scan_tolerance(N, total):
    m = scan_roundings(N)
    return (m * U / (1 - m * U) + U) * total       # + u: the reference's rounding


@pytest.mark.parametrize("N", SCAN_N)
@pytest.mark.parametrize("family", SCAN_FAMILIES)
def test_scan_is_a_cdf(dev, family, N):
    """P1  nondecreasing.
    P2  out[i] == out[i-1] wherever w[i] == 0, and out[0] == w[0].
    P3  |out[i] - exact[i]| <= m u / (1 - m u) exact[N-1], m =
        scan_roundings(N): a sum of non-negative terms in which no term meets
        more than m roundings (K = m / 2 in eps: 132.5 up to N = 2048, 260.5
        at N = 524289).
    A positive weight absorbed by a much larger prefix (out[i] == out[i-1]
    with w[i] > 0) is allowed.  Bitwise reproducible."""
    from pyabc_amd import gpu
    w = scan_family(family, N)
    ref = cached(("scan", family, N), lambda: wx.exact_prefix(w).values)
    wd = T(w)
    out = gpu.inclusive_scan(wd).cpu().numpy()
    drops = np.nonzero(np.diff(out) < 0)[0]
    assert len(drops) == 0, (len(drops), drops[:5])                        # P1
    assert out[0] == w[0]                                                  # P2
    rises = np.nonzero((w[1:] == 0) & (out[1:] != out[:-1]))[0]
    assert len(rises) == 0, (len(rises), rises[:5])
    err = np.abs(out - ref)
    tol = scan_tolerance(N, ref[-1])
    assert (err <= tol).all(), err.max() / tol                             # P3
    assert np.array_equal(gpu.inclusive_scan(wd).cpu().numpy(), out)
    report(f"scan {family} N={N}", scan_roundings(N) / 2, err.max() / (EPS * ref[-1]))


# ---- ancestor draws against the exact cdf ---------------------------------------------

def anc_weights(family, N):
    rng = np.random.default_rng(5000 + N)
    w = rng.uniform(size=N)
    if family == "zeros":
        w[rng.uniform(size=N) < 0.7] = 0.0
        if N > 12:
            w[:5] = 0.0
            w[-5:] = 0.0
        w[N // 2] = 0.625
    elif family == "dominant":
        w[N // 3] = 1e6
    elif family == "decades":
        w = 10.0 ** rng.uniform(-300.0, 0.0, N)
    return w


@pytest.mark.parametrize("mode", ["mvn", "local"])
@pytest.mark.parametrize("N", [1, 2, 65, 4000])
@pytest.mark.parametrize("family", ["zeros", "dominant", "decades"])
def test_ancestors_against_the_exact_cdf(dev, family, N, mode):
    """The plain search, the cdf-guide search and the ancestor-table search
    (the fused rounds' proposal) on B = 40000 draws.  Each draw's uniform u is
    recovered from its Philox stream; with t = u x (the scan's total) the
    ancestor j must satisfy, on the EXACT cdf of the weights,

        exact[j-1] - tol <= t <= exact[j] + tol,    tol = the scan's P3 bound

    (the device found cdf[j-1] <= t < cdf[j] on a scan within tol of exact).
    No row of weight 0 is ever drawn; the three searches agree."""
    from pyabc_amd import gpu
    from test_gpu_fused import _case, _round
    d, B, lo, seed, gen = 3, 40_000, 99, 11, 3
    c = _case(d, 3, N=N, mode="mvn" if mode == "mvn" else "local", seed=4)
    w = anc_weights(family, N)
    ref = cached(("anc", family, N), lambda: wx.exact_prefix(w).values)
    cdf = gpu.inclusive_scan(T(w))
    c.update(cdf=cdf, guide=gpu.cdf_guide(cdf))
    args = (c["X"], cdf, c["L"], c["kind"], c["params"], seed, gen, lo, B, 1000, d)
    _, _, a_plain, att = gpu.propose(*args, per_particle_L=c["ppl"])
    _, _, a_guide, _ = gpu.propose(*args, per_particle_L=c["ppl"], guide=c["guide"])
    _, _, a_table, _ = _round(c, seed=seed, gen=gen).propose(lo, B)
    assert torch.equal(a_plain, a_guide) and torch.equal(a_plain, a_table)
    assert int(att.max()) == 1          # normal priors: the first attempt stands
    j = a_plain.cpu().numpy()
    assert j.min() >= 0 and j.max() < N
    assert (w[j] > 0).all()
    r = philox4x32_10(np.arange(lo, lo + B, dtype=np.uint64), 0, gen, seed)
    t = uniform53(r[:, 0], r[:, 1]) * float(cdf[-1].item())
    tol = scan_tolerance(N, ref[-1])
    below = np.where(j > 0, ref[np.maximum(j - 1, 0)], 0.0)
    assert (below - tol <= t).all() and (t <= ref[j] + tol).all()
    if family == "dominant" and N > 2:
        assert (j == N // 3).mean() > 0.9
