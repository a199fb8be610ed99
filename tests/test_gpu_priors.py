"""The prior layer of pyabc_amd/csrc/abc_candidate.h against independent
references: the t = 0 draw (prior_draw1 / gamma_draw) against the oracle's
stream-for-stream replay, whose own draws tests/test_oracle_priors.py holds
to scipy's cdfs; the support box (abc_prior_support_box) against a host
bisection over scipy's density and against the device's own density; the
density (prior_logpdf1) against scipy at the points where its special cases
sit; and one ABCSMC run with gamma / beta / lognorm / laplace priors.

Where scipy's own logpdf is wrong the tests say so and hold the device to
the closed form instead (_SCIPY_LOSES below): scipy.stats.laplace.logpdf is
log(pdf) and underflows to -inf for |y| > 745; scipy.stats.lognorm.logpdf
takes log(s y sqrt(2 pi)) of a product that overflows for y > 7e307 / s and
is rounded (to 0 for s <= 0.79) for a subnormal y.
"""
import itertools

import numpy as np
import pytest
from scipy import stats

import oracle
import oracle.sampler as osamp
from test_oracle_priors import NSHAPE, SHAPES, frozen

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INF = np.inf


@pytest.fixture(scope="module")
def dev():
    from pyabc_amd import gpu
    return gpu.require_device()


def T(a, dtype=None):
    from pyabc_amd import gpu
    return gpu.as_dev(a, dtype=dtype)


def _spec(cols):
    """Device (kind [d] int32, params [4 d]) of [(kind name, params)]."""
    kinds = T([osamp.KIND[k] for k, _ in cols], dtype=torch.int32)
    params = np.zeros((len(cols), 4))
    for i, (_, p) in enumerate(cols):
        params[i, :len(p)] = p
    return kinds, T(params.ravel())


def _round(cols, seed, generation, max_attempts):
    """A CandidateRound over the prior alone (one dummy statistic)."""
    from pyabc_amd import gpu
    kinds, params = _spec(cols)
    one = T(np.ones(1))
    return gpu.CandidateRound(len(cols), 1, kinds, params, T([0], dtype=torch.int32), one, one,
                              one, one, 2.0, seed, generation, max_attempts)


# ---- a. the t = 0 draw -------------------------------------------------------

# every shape of the oracle's KS test plus a lognorm whose exp(s n) leaves the
# doubles for |n| > 3.55 (about 4e-4 of the draws): those rows are re-drawn
WIDE_LOGNORM = ("lognorm", [200.0, 0.0, 1.0, 0.0])
COLS = SHAPES + [WIDE_LOGNORM]
LAYOUTS = {
    # runtime-d kernel; a beta with shapes < 1 in front of a gamma
    7: [COLS[i] for i in (0, 6, 1, 9, 16, 12, 5)],
    # templated kernel: all but the first gamma
    16: COLS[1:],
    # propose_wide_kernel: every shape four times over, slots up to 32 + 512 * 69
    70: [COLS[k % len(COLS)] for k in range(70)],
}
REPLAY_SEED = 9
_replay_cache = {}


def _replay(d, idx0, B, max_attempts):
    key = (d, idx0)
    if key not in _replay_cache:
        cols = LAYOUTS[d]
        ref = osamp.propose_prior([k for k, _ in cols], np.array([p for _, p in cols]),
                                  REPLAY_SEED, 0, idx0, B, max_attempts)
        for a in ref:
            a.setflags(write=False)
        _replay_cache[key] = ref
    return _replay_cache[key]


@pytest.mark.parametrize("idx0", [0, 2 ** 32 + 12345])
@pytest.mark.parametrize("d", [7, 16, 70])
def test_prior_draw_replay(dev, d, idx0):
    """gpu.propose in prior mode == the oracle's replay, candidate for
    candidate: attempts equal, theta within 1e-12 (relative to the larger of
    |theta| and |loc|: the final loc + scale x rounds relative to its larger
    operand), log density within rtol 1e-10 with the same infinities.  No
    candidate is left out: instead the replay's smallest Marsaglia-Tsang
    accept margin |log u - rhs| must be >= 1e-9, far above the ~1e-15 by
    which the device's log can differ from numpy's, so no accept decision
    can differ.  The wide lognorm makes attempts == 2 rows.  For d <= 64 the
    fused proposal kernel (CandidateRound.propose) returns the same bits.

    Measured on an MI355X (seed 9, printed below): theta error at most
    6.5e-16, log density error at most 8.7e-13 but for one d = 16 row whose
    terms cancel to |lp| = 4.5e-4 (6.3e-11), smallest accept margin 3.1e-7,
    0 to 7 re-drawn rows per case."""
    from pyabc_amd import gpu
    B, max_attempts = 4096, 10
    cols = LAYOUTS[d]
    th_o, lp_o, att_o, margin = _replay(d, idx0, B, max_attempts)
    kinds, params = _spec(cols)
    th, lp, _, att = gpu.propose(None, None, None, kinds, params, REPLAY_SEED, 0, idx0, B,
                                 max_attempts, d)
    th_h, lp_h, att_h = th.cpu().numpy(), lp.cpu().numpy(), att.cpu().numpy()
    loc = np.array([p[NSHAPE[k]] for k, p in cols])
    scale = np.maximum(np.abs(th_o), np.abs(loc)[None, :])
    err_th = np.abs(th_h - th_o) / scale
    fin = np.isfinite(lp_o)
    err_lp = np.abs(lp_h[fin] - lp_o[fin]) / np.abs(lp_o[fin])
    print(f"d={d} idx0={idx0}: margin {margin.min():.3e}  theta err {np.nanmax(err_th):.3e}  "
          f"lp err {err_lp.max():.3e}  redrawn {(att_o > 1).sum()}")
    assert margin.min() >= 1e-9
    np.testing.assert_array_equal(att_h, att_o)
    assert np.isfinite(th_o).all() and (err_th <= 1e-12).all(), np.nanmax(err_th)
    np.testing.assert_array_equal(np.isfinite(lp_h), fin)
    np.testing.assert_array_equal(lp_h[~fin], lp_o[~fin])
    np.testing.assert_allclose(lp_h[fin], lp_o[fin], rtol=1e-10, atol=0)
    assert (att_o <= max_attempts).all()
    if d == 70:
        assert (att_o == 2).any()          # the re-draw loop ran
    if d <= 64:
        fr = _round(cols, REPLAY_SEED, 0, max_attempts)
        th2, lp2, _, att2 = fr.propose(idx0, B)
        assert torch.equal(th2, th) and torch.equal(lp2, lp) and torch.equal(att2, att)


def test_prior_draw_gives_up_like_replay(dev):
    """max_attempts = 1: the rows the wide lognorm throws out give up
    (attempts 2, log density -inf, theta the rejected draw) exactly where the
    replay's do, in the staged and the fused kernel."""
    from pyabc_amd import gpu
    cols = [("norm", [0.0, 1.0]), WIDE_LOGNORM, ("gamma", [0.5, 0.0, 1.0])]
    B = 50_000
    th_o, lp_o, att_o, _ = osamp.propose_prior([k for k, _ in cols],
                                               [list(p) + [0.0] * (4 - len(p)) for _, p in cols],
                                               3, 0, 77, B, 1)
    kinds, params = _spec(cols)
    th, lp, _, att = gpu.propose(None, None, None, kinds, params, 3, 0, 77, B, 1, 3)
    out = att_o == 2
    assert 5 <= out.sum() <= 60       # 50 000 * 3.9e-4 = 19.5 expected
    np.testing.assert_array_equal(att.cpu().numpy(), att_o)
    assert np.isneginf(lp.cpu().numpy()[out]).all()
    np.testing.assert_array_equal(th.cpu().numpy()[out, 1], th_o[out, 1])   # 0 or inf
    fr = _round(cols, 3, 0, 1)
    th2, lp2, _, att2 = fr.propose(77, B)
    assert torch.equal(th2, th) and torch.equal(lp2, lp) and torch.equal(att2, att)


# ---- b. the support box ------------------------------------------------------

def _support_box(cols):
    """abc_prior_support_box of [(kind name, params)]: [n, 2] (lo, hi)."""
    from pyabc_amd import _native as nat
    from pyabc_amd import gpu
    out = []
    for i in range(0, len(cols), 64):
        part = cols[i:i + 64]
        kinds, params = _spec(part)
        box = torch.empty(2 * len(part), dtype=torch.float64, device=params.device)
        nat.call("abc_prior_support_box", gpu.p(kinds), gpu.p(params), len(part), gpu.p(box),
                 gpu.stream_ptr())
        out.append(box.cpu().numpy().reshape(-1, 2))
    return np.concatenate(out)


def _device_logpdf1(col, x):
    """prior_logpdf1 of one (kind, params) at the points x."""
    from pyabc_amd import gpu
    kinds, params = _spec([col])
    return gpu.prior_logpdf(T(np.asarray(x, dtype=np.float64).reshape(-1, 1)), kinds,
                            params).cpu().numpy()


def _key(x):
    """Order-preserving uint64 image of a double (as a Python int)."""
    u = int(np.float64(x).view(np.uint64))
    return (~u) & (2 ** 64 - 1) if u >> 63 else u | (1 << 63)


def _val(k):
    u = k & ~(1 << 63) if k >> 63 else (~k) & (2 ** 64 - 1)
    return float(np.uint64(u).view(np.float64))


def _host_box(member, c):
    """[lowest, highest] double x with member(x), by bisection over the
    ordered keys on either side of the member c."""
    assert member(c)
    if member(-INF):
        lo = -INF
    else:
        a, b = _key(-INF), _key(c)          # member(a) false, member(b) true
        while b - a > 1:
            m = (a + b) // 2
            if member(_val(m)):
                b = m
            else:
                a = m
        lo = _val(b)
    if member(INF):
        hi = INF
    else:
        a, b = _key(c), _key(INF)           # member(a) true, member(b) false
        while b - a > 1:
            m = (a + b) // 2
            if member(_val(m)):
                a = m
            else:
                b = m
        hi = _val(a)
    return lo, hi


def _scipy_member(col):
    fr = frozen(*col)
    with np.errstate(all="ignore"):
        return lambda x: bool(fr.logpdf(x) > -INF)


# Families whose scipy logpdf returns -inf inside the support (module
# docstring): membership by the closed form of the same density instead,
#   laplace  log f = -|y| - log(2 scale)            finite iff y is
#   lognorm  log f = -(log y / s)^2 / 2 - log y - log(s scale sqrt(2 pi))
#                                                   finite iff 0 < y < inf
# with y = (x - loc) / scale in float64 as scipy computes it.
def _y(col, x):
    kind, p = col
    with np.errstate(all="ignore"):
        return (np.float64(x) - np.float64(p[NSHAPE[kind]])) / np.float64(p[NSHAPE[kind] + 1])


_SCIPY_LOSES = {
    "laplace": lambda col: (lambda x: bool(np.isfinite(_y(col, x)))),
    "lognorm": lambda col: (lambda x: bool(0.0 < _y(col, x) < INF)),
}


def _grid_cols(locs_scales, shapes=(0.5, 1.0, 2.0)):
    cols = []
    for loc, sc in locs_scales:
        for k in ("norm", "uniform", "expon", "laplace"):
            cols.append((k, [loc, sc]))
        for s in shapes:
            cols.append(("lognorm", [s, loc, sc]))
            cols.append(("gamma", [s, loc, sc]))
        for a, b in itertools.product(shapes, shapes):
            cols.append(("beta", [a, b, loc, sc]))
    return cols


ORDINARY = _grid_cols(list(itertools.product([0.0, -3.5, 1e6], [1e-3, 1.0, 7.25])))
SUBNORMAL = 1e-320
EXTREME = _grid_cols([(0.0, 1e-300), (-3.5, 1e-300), (0.0, 1e300), (-3.5, 1e300),
                      (1e20, 1.0), (-1e20, 1.0), (0.0, SUBNORMAL), (1.0, SUBNORMAL)])


def _check_box_against_device_density(cols, box):
    """Reference 2: the density the device evaluates is > -inf at both ends
    of the box and -inf (or NaN) at the doubles just outside; an empty box
    has no member at loc, the doubles next to it, or loc + scale (/ 2)."""
    empty = 0
    for col, (lo, hi) in zip(cols, box):
        kind, p = col
        if lo > hi:
            assert (lo, hi) == (INF, -INF), (col, lo, hi)
            loc, sc = np.float64(p[NSHAPE[kind]]), np.float64(p[NSHAPE[kind] + 1])
            with np.errstate(all="ignore"):
                x = [loc, np.nextafter(loc, -INF), np.nextafter(loc, INF), loc + sc,
                     loc + 0.5 * sc, np.nextafter(loc + sc, -INF)]
            lp = _device_logpdf1(col, x)
            assert not (lp > -INF).any(), (col, x, lp)
            empty += 1
            continue
        x = [lo, hi]
        with np.errstate(over="ignore"):     # next to the largest double: inf
            if lo > -INF:
                x.append(np.nextafter(lo, -INF))
            if hi < INF:
                x.append(np.nextafter(hi, INF))
        lp = _device_logpdf1(col, x)
        assert (lp[:2] > -INF).all(), (col, lo, hi, lp)
        assert not (lp[2:] > -INF).any(), (col, lo, hi, x, lp)
    return empty


def test_prior_support_box(dev):
    """abc_prior_support_box against (1) the host bisection over scipy's
    membership logpdf(x) > -inf, value for value (-0.0 == 0.0: both zeros are
    the same point), on the ordinary grid; (2) the device's own density at
    and next to the box's ends, on the ordinary and the extreme grid."""
    box = _support_box(ORDINARY)
    nested = 0
    for col, (lo, hi) in zip(ORDINARY, box):
        kind = col[0]
        fr = frozen(*col)
        c = float(fr.ppf(0.5))
        ref = _host_box(_scipy_member(col), c)
        if kind in _SCIPY_LOSES:
            # scipy's members are members, and the box is the closed form's
            assert lo <= ref[0] and ref[1] <= hi, (col, (lo, hi), ref)
            if kind == "lognorm":
                assert lo == ref[0], (col, lo, ref)
            nested += (lo, hi) != ref
            ref = _host_box(_SCIPY_LOSES[kind](col), c)
        assert (lo, hi) == ref, (col, (lo, hi), ref)
    # the listed scipy losses are real: drop the entry once scipy has none
    assert nested > 0
    assert _check_box_against_device_density(ORDINARY, box) == 0


def test_prior_support_box_extreme(dev):
    """Reference 2 on scales 1e-300 / 1e300 / subnormal and loc = +-1e20 with
    scale 1 -- where loc + scale rounds onto loc: gamma(2, 1e20, 1) has the
    support (1e20, DBL_MAX], which the bisection used to report empty -- and
    the closed-form box for the kinds whose box is plain; an infinite uniform
    scale and NaN parameters have no density anywhere: the empty box."""
    box = _support_box(EXTREME)
    empty = _check_box_against_device_density(EXTREME, box)
    by = dict(((k, tuple(p)), tuple(b)) for (k, p), b in zip(EXTREME, box))
    big = float(np.finfo(np.float64).max)
    up = float(np.nextafter(1e20, INF))
    assert by[("gamma", (2.0, 1e20, 1.0))] == (up, big)
    assert by[("gamma", (1.0, 1e20, 1.0))] == (1e20, big)
    assert by[("lognorm", (1.0, 1e20, 1.0))] == (up, big)
    assert by[("expon", (1e20, 1.0))] == (1e20, big)
    assert by[("uniform", (1e20, 1.0))] == (1e20, 1e20)
    assert by[("beta", (0.5, 0.5, 1e20, 1.0))] == (1e20, 1e20)
    assert by[("beta", (2.0, 0.5, 1e20, 1.0))] == (INF, -INF)    # no double inside
    assert by[("beta", (2.0, 2.0, -1e20, 1.0))] == (INF, -INF)
    assert by[("gamma", (2.0, -1e20, 1.0))] == (float(np.nextafter(-1e20, INF)), big)
    assert by[("norm", (0.0, 1e300))] == (-big, big)
    assert by[("laplace", (-3.5, 1e300))] == (-big, big)
    # empty only where no double lies inside: beta with a vanishing end point
    for (kind, p), b in zip(EXTREME, box):
        if tuple(b) == (INF, -INF):
            assert kind == "beta" and (p[0] > 1.0 or p[1] > 1.0), (kind, p)
    assert empty > 0
    bad = [("uniform", [0.0, INF]), ("uniform", [-3.5, INF])]
    for k in ("norm", "uniform", "expon", "laplace"):
        bad += [(k, [np.nan, 1.0]), (k, [0.0, np.nan])]
    for k in ("lognorm", "gamma"):
        bad += [(k, [np.nan, 0.0, 1.0]), (k, [2.0, np.nan, 1.0]), (k, [2.0, 0.0, np.nan])]
    bad += [("beta", [2.0, 2.0, np.nan, 1.0]), ("beta", [2.0, 2.0, 0.0, np.nan])]
    bbox = _support_box(bad)
    for col, b in zip(bad, bbox):
        assert tuple(b) == (INF, -INF), (col, b)
        lp = _device_logpdf1(col, [0.0, 0.5, 1.0, -3.5, 1e300, INF])
        assert not (lp > -INF).any(), (col, lp)


# ---- c. the density at its edges -----------------------------------------------

def _edge_points(col):
    kind, p = col
    loc, sc = np.float64(p[NSHAPE[kind]]), np.float64(p[NSHAPE[kind] + 1])
    up = loc + sc
    return np.array([loc, np.nextafter(loc, -INF), np.nextafter(loc, INF),
                     up, np.nextafter(up, -INF), np.nextafter(up, INF),
                     loc + sc * 1e-300, loc + sc * 1e300, -INF, INF, loc + 0.3 * sc])


def _closed_form(col, x):
    """log f of the two _SCIPY_LOSES families, in long double (64-bit
    mantissa, 15-bit exponent: no overflow or subnormal in these terms)."""
    kind, p = col
    ld = np.longdouble
    y = np.asarray(_y(col, x)).astype(ld)
    with np.errstate(all="ignore"):
        if kind == "laplace":
            return (-np.abs(y) - np.log(ld(2.0) * ld(p[1]))).astype(np.float64)
        s, sc = ld(p[0]), ld(p[2])
        ly = np.log(y)
        out = -(ly / s) ** 2 / 2 - ly - np.log(s * sc * np.sqrt(2 * ld(np.pi)))
        return np.where(y > 0, out, -INF).astype(np.float64)


def _edge_reference(col):
    """scipy's frozen logpdf at the edge points; where scipy is off the
    closed form (module docstring) the closed form.  Returns (x, ref, number
    of points taken from the closed form)."""
    x = _edge_points(col)
    with np.errstate(all="ignore"):
        ref = np.asarray(frozen(*col).logpdf(x), dtype=np.float64)
    taken = 0
    if col[0] in _SCIPY_LOSES:
        exact = _closed_form(col, x)
        with np.errstate(all="ignore"):
            off = ~((ref == exact) | (np.abs(ref - exact) <= 1e-12 * np.abs(exact)))
        y = _y(col, x)
        # only where the loss is understood: laplace |y| > 745, lognorm y
        # subnormal (< 2.3e-308)
        known = (np.abs(y) > 745.0) if col[0] == "laplace" else ((y > 0) & (y < 2.3e-308))
        assert not (off & ~known).any(), (col, x[off & ~known], ref, exact)
        ref = np.where(off, exact, ref)
        taken = int(off.sum())
    return x, ref, taken


def _assert_like(got, ref, what):
    for test in (np.isnan, np.isposinf, np.isneginf):
        np.testing.assert_array_equal(test(got), test(ref), err_msg=str(what))
    fin = np.isfinite(ref)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-10, atol=1e-13, err_msg=str(what))


EDGE = _grid_cols([(0.0, 1.0), (-3.5, 7.25), (1e6, 1e-3)])


def test_prior_logpdf_edges_vs_scipy(dev):
    """gpu.prior_logpdf == scipy's frozen logpdf (same NaN / +inf / -inf,
    finite values at rtol 1e-10, atol 1e-13) at loc, the upper end point loc +
    scale, the doubles next to each, y = 1e-300, y = 1e300 and +-inf, for
    the seven families (shapes in {0.5, 1, 2}) and flat: gamma at y == 0 on
    either side of a = 1, beta's a == 1 / b == 1 shortcuts and end points,
    the overflow ends.  d = 3 with the case in each column in turn, and
    d = 80 (all cases side by side).  On the same points, membership by
    prior_logpdf > -inf is membership by the support box."""
    from pyabc_amd import gpu
    box = _support_box(EDGE)
    refs = [_edge_reference(col) for col in EDGE]
    assert sum(t for _, _, t in refs) > 0      # drop _SCIPY_LOSES once this is 0
    side = [("norm", [0.0, 1.0]), ("flat", [])]
    side_lp = stats.norm.logpdf(0.3)
    for i, (col, (x, ref, _), (lo, hi)) in enumerate(zip(EDGE, refs, box)):
        cols = list(side)
        cols.insert(i % 3, col)
        th = np.full((len(x), 3), 0.3)
        th[:, i % 3] = x
        kinds, params = _spec(cols)
        got = gpu.prior_logpdf(T(th), kinds, params).cpu().numpy()
        _assert_like(got, ref + side_lp if i % 3 == 0 else side_lp + ref, col)
        np.testing.assert_array_equal(got > -INF, (lo <= x) & (x <= hi), err_msg=str(col))
    # runtime d = 80: the cases side by side, row r = everyone's point r
    for i in range(0, len(EDGE), 80):
        part = list(range(i, min(i + 80, len(EDGE))))
        part += [part[-1]] * (80 - len(part))
        th = np.stack([refs[k][0] for k in part], axis=1)
        want = np.zeros(th.shape[0])
        with np.errstate(invalid="ignore"):
            for k in part:
                want = want + refs[k][1]
        kinds, params = _spec([EDGE[k] for k in part])
        got = gpu.prior_logpdf(T(th), kinds, params).cpu().numpy()
        _assert_like(got, want, ("d = 80 from case", i))
    # flat: 0 everywhere, and the whole line is its box
    x = np.array([0.0, -1e300, 1e300, -INF, INF])
    np.testing.assert_array_equal(_device_logpdf1(("flat", []), x), np.zeros(5))
    assert tuple(_support_box([("flat", [])])[0]) == (-INF, INF)


# ---- d. end to end ---------------------------------------------------------------

def test_abcsmc_with_shaped_priors(dev):
    """ABCSMC with gamma (a < 1), beta (b < 1), lognorm and laplace priors
    built positionally, by keyword and mixed: generation 0 (eps = inf: its
    particles are the first prior draws) passes a KS test per margin
    against scipy (1.95 / sqrt(N): the 0.1 % critical value), and at t = 1, 2
    every stored weight is prior.pdf / transition.pdf of the stored previous
    population up to normalisation (scipy priors, oracle.mvn_logpdf; 2e-6,
    the x3 density's bar in test_step_golden)."""
    import pyabc_amd as pa
    N = 2000
    prior = pa.Distribution(a=pa.RV("gamma", 0.7, scale=2), b=pa.RV("beta", 2, 0.6),
                            c=pa.RV("lognorm", s=0.5), d=pa.RV("laplace", 1, 0.5))
    names = ["a", "b", "c", "d"]
    model = pa.LinearGaussianModel(names, ["y0", "y1", "y2", "y3"], src=[0, 1, 2, 3],
                                   sigma=[0.5] * 4)
    abc = pa.ABCSMC(model, prior, pa.PNormDistance(), population_size=N,
                    sampler=pa.BatchedGPUSampler(seed=4321),
                    eps=pa.QuantileEpsilon(initial_epsilon=np.inf, alpha=0.5))
    abc.new("sqlite://", {"y0": 1.5, "y1": 0.7, "y2": 1.0, "y3": 1.2})
    h = abc.run(minimum_epsilon=-1, max_nr_populations=3)
    assert h.max_t == 2
    sp = dict(a=stats.gamma(0.7, scale=2), b=stats.beta(2, 0.6), c=stats.lognorm(0.5),
              d=stats.laplace(1, 0.5))
    df0, w0 = h.get_distribution(0, 0)
    assert len(df0) == N
    np.testing.assert_allclose(w0, 1.0 / N, rtol=1e-12)
    for n in names:
        ks = stats.kstest(df0[n].values, sp[n].cdf).statistic
        assert ks < 1.95 / np.sqrt(N), (n, ks)
    prev, wprev = df0, w0
    for t in (1, 2):
        df, w = h.get_distribution(0, t)
        assert len(df) == N
        X = prev[names].values
        cov, wn = oracle.mvn_fit(X, np.asarray(wprev))
        th = df[names].values
        lt = oracle.mvn_logpdf(th, X, wn, cov)
        lp = sum(sp[n].logpdf(th[:, k]) for k, n in enumerate(names))
        assert np.isfinite(lp).all()
        lw = lp - lt
        ref = np.exp(lw - lw.max())
        ref /= ref.sum()
        np.testing.assert_allclose(np.asarray(w), ref, rtol=2e-6, atol=0)
        prev, wprev = df, w
