"""The weighted quantile that sets eps (abc_weighted_quantile, the weighted
MSD select of abc_quantile.hip, and abc_weighted_quantile_sorted, its
sort-based fallback) against the exact reference of oracle/quantile_exact.py:
both launch paths (one resident-grid launch up to 2^20 points, several
launches above), every grid shape of the hand-off arithmetic, every data shape
on both paths, the edges of the key and weight ranges, the calls as a
sequence on one workspace, and the calls QuantileEpsilon makes.

Tolerance model
---------------
Dyadic weights (integers over a power of two, oracle.quantile_exact.
dyadic_weights) and finite knots: every sum any kernel forms is exact, xp is
exact, and the only rounding left is slope * (alpha - xp_j) + y_j:

    |q - q_exact| <= 4 ulp(max(|y_j|, |y_j1|)),

and q equals q_exact as a number wherever it is a copy of one input point (a
clamp, an exact knot hit, the last knot) or infinite.  (-0.0 and +0.0 are one
key in both kernels; q carries +0.0 for either.)

General weights:

    |q - q_exact| <= 1e-12 |q_exact| + N eps |y_j1 - y_j| / (xp_j1 - xp_j),

the worst-case rounding of a sum of N non-negative terms pushed through the
interpolation slope.  It is loose, but a wrong knot errs by the order of
|y_j1 - y_j| and N^2 eps <= 2^-12 for every N here, so it still tells the
two apart.  tests/test_oracle_quantile_exact.py shows that numpy's float64
oracle meets both rules on the same inputs (it uses up to 0.08 of the general
budget: a sequential cumsum of equal weights rounds the same way N times).

Measured share of the general budget used on the device (MI355X,
test_general_weights, largest over cases and alphas):
    one launch (N = 36 865):          select 3.3e-5, sorted 2.2e-4
    several launches (N = 2^20 + 1):  select 1.1e-6, sorted 1.8e-4

What fails when a hand-off or boundary is wrong
-----------------------------------------------
* a group count from min(gridDim, 8), a group size from (gridDim - g + 7) >> 3:
  test_grid_shapes at 2, 8, 9 and 10 blocks (N = 4097 .. 9 * 4096 + 5) -- a
  wrong count releases a stage before every block's histogram has arrived
  (wrong q) or never (NaN: the test demands a decided result);
* a WQ_REFINE / WQ_CAP comparison: test_list_sizes, whose segment is the whole
  input at N = 256, 257, 2048 (decided: both rank-sort layouts and a full
  list) and 2049 (NaN, sorted kernel answers); test_shapes[dense_core] above
  2^20, which needs every level of the multi-launch path;
* the margin in the pick: test_weight_geometry[staircase] -- half the weights
  lose 0.9 of their ~1.9 fixed-point units, so the truncated cumulative
  weight at a knot in the other half is ~N / 9000 points short of alpha x
  total; with a zero margin the segment misses the knots (checked: that
  mutant fails this test and, of the others, only test_list_sizes[2049]).
  test_weight_geometry[dominant] and test_general_weights[exp6] run the pick
  where most fixed-point weights are 1 or 0 units;
* seg_keys' clamp at hi: test_key_geometry[inf30] -- the keys end at +inf's
  0xfff0..., so the last bin's end lo + off passes 2^64 without the clamp;
* the at_start / at_end clamps: alpha = 0, 1 and the alphas outside
  [xp_0, xp_{N-1}] of every test, bit-equal, and test_weight_geometry
  [edge_zeros], where the clamp must not fire although alpha = 0 and 1;
* the control-block reset after an undecided call: test_call_sequence.
"""
import types

import numpy as np
import pytest

import oracle.quantile_exact as qe

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_ONE, N_FOUR, N_FOUR_B = 36_865, (1 << 20) + 1, (1 << 20) + 4097
PATH = {N_ONE: "one", N_FOUR: "several", N_FOUR_B: "several"}


@pytest.fixture(scope="module")
def dev():
    from pyabc_amd import gpu
    return gpu.require_device()


def T(a):
    from pyabc_amd import gpu
    return gpu.as_dev(a)


def run(P, W, alphas, sorted_path=False):
    """Every alpha queued on the stream, one read."""
    from pyabc_amd import gpu
    qs = [gpu.weighted_quantile(P, W, a, sorted_path=sorted_path) for a in alphas]
    return torch.cat(qs).cpu().numpy()


SHARE = {}   # (path, kernel) -> largest share of the general budget used


def within(q, r, N, dyadic, tag):
    if dyadic:
        tol = qe.budget_dyadic(r)
        if tol == 0.0:
            assert qe.same_value(q, r.q), (tag, q, r)
        else:
            assert abs(q - r.q) <= tol, (tag, q, r, abs(q - r.q) / qe.ulp_max(r))
    else:
        tol, _ = qe.budget_general(r, N)
        err = abs(q - r.q)
        if tol > 0:
            key = (PATH.get(N, "one"), tag[0])
            SHARE[key] = max(SHARE.get(key, 0.0), err / tol)
        assert err <= tol, (tag, q, r, err, tol)


def check(case, N, pts, w, ref, alphas, dyadic=True, decided=None, sorted_too=True):
    """The select at every alpha (raw: NaN = undecided), the sorted kernel on
    the same input, both against the exact reference.  decided: True, or a
    predicate of alpha -- where it holds the select itself must answer."""
    P, W = T(pts), T(w)
    raw = run(P, W, alphas)
    srt = run(P, W, alphas, sorted_path=True) if sorted_too else None
    undecided = []
    for i, a in enumerate(alphas):
        r = ref(a)
        must = decided(a) if callable(decided) else bool(decided)
        if must:
            assert not np.isnan(raw[i]), (case, N, a, "the select must decide")
        if np.isnan(raw[i]):
            undecided.append(a)
            assert srt is not None, (case, N, a, "undecided")
        else:
            within(raw[i], r, N, dyadic, ("select", case, N, a))
        if srt is not None:
            within(srt[i], r, N, dyadic, ("sorted", case, N, a))
    return raw, undecided


def extra_alphas(case, ref, m):
    if case == "inf30":
        return qe.inf_alphas(ref)
    return ()


# ---- a. grid shapes of the one-launch path ---------------------------------------

@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 2048, 2049, 4096, 4097,
                               7 * 4096 + 1, 8 * 4096, 8 * 4096 + 1, 9 * 4096 + 5,
                               65 * 4096 - 5, 1 << 20])
def test_grid_shapes(dev, N):
    """1, 2, 8, 9, 10, 65 and 256 blocks, a ragged last chunk: continuous
    points, dyadic flat weights, every alpha decided by the select."""
    rng = qe.seed(f"grid:{N}")
    pts = qe.points_recipe(rng, N, "normal")
    w, m, _ = qe.dyadic_weights(rng, N, "flat")
    ref = qe.ExactQuantile(pts, m)
    check("grid", N, pts, w, ref, qe.alpha_set(ref), decided=True, sorted_too=False)


@pytest.mark.parametrize("N", [256, 257, 2048, 2049])
def test_list_sizes(dev, N):
    """One low point and N - 1 ties: the segment always keeps the low point's
    bin, so the list holds exactly N points at every alpha -- WQ_REFINE, one
    more (refined, the other rank-sort layout), WQ_CAP (full list), one more
    (undecided: NaN, and the sorted kernel answers).  The value between the
    low point and the first tie by index depends on the stable order of the
    list (alpha_set's midpoint above knot 0)."""
    rng = qe.seed(f"list:{N}")
    pts = np.full(N, 2.0)
    pts[N // 2] = 1.0
    w, m, _ = qe.dyadic_weights(rng, N, "flat")
    ref = qe.ExactQuantile(pts, m)
    assert ref.order[1] == 0 and ref(ref.knot(0) / 2 + ref.knot(1) / 2).yj1 == 2.0
    raw, undecided = check("list", N, pts, w, ref, qe.alpha_set(ref), decided=(N <= 2048))
    if N == 2049:
        assert np.isnan(raw).all()


# ---- b. every data shape on both paths ---------------------------------------------

@pytest.mark.parametrize("N", [N_ONE, N_FOUR, N_FOUR_B])
@pytest.mark.parametrize("case", list(qe.SHAPE_CASES))
def test_shapes(dev, case, N):
    """The data shapes of test_weighted_quantile_select at 10 blocks of the
    one-launch path and on the multi-launch path (its 2048-bin level-1 pick,
    its early exits, its NaN hand-over to the sorted kernel).  Continuous
    data, zero weights and dense_core are decided by the select itself; ties
    by the thousand may come back NaN and are then answered by the sorted
    kernel, which runs on every input anyway."""
    pts, w, m = qe.dyadic_case(case, N)
    ref = qe.ExactQuantile(pts, m)
    check(case, N, pts, w, ref, qe.alpha_set(ref), decided=case in qe.SHAPE_DECIDED)


# ---- c. key geometry ------------------------------------------------------------------

@pytest.mark.parametrize("N", [N_ONE, N_FOUR])
@pytest.mark.parametrize("case", list(qe.KEY_CASES))
def test_key_geometry(dev, case, N):
    """Mixed signs, a span over nearly all 64 key bits, subnormals with both
    zeros, one key only, one value between +-1e300, +inf distances."""
    pts, w, m = qe.dyadic_case(case, N)
    ref = qe.ExactQuantile(pts, m)
    alphas = qe.alpha_set(ref, extra=extra_alphas(case, ref, m))
    decided = {"symmetric": True, "wide": True,
               "subnormal": N == N_ONE,
               # finite knots well below the inf run (which starts near 0.7)
               "inf30": lambda a: a <= 0.6}.get(case)
    raw, undecided = check(case, N, pts, w, ref, alphas, decided=decided)
    if case == "inf30":
        inside, last_finite, first_inf, mid = [ref(a) for a in alphas[-4:]]
        assert inside.q == first_inf.q == mid.q == np.inf
        assert last_finite.copy and np.isfinite(last_finite.q)
    if case == "zeros_pm":
        assert np.isnan(raw).all()          # N equal keys: never decided


# ---- d. weight geometry ---------------------------------------------------------------

@pytest.mark.parametrize("N", [N_ONE, N_FOUR])
@pytest.mark.parametrize("case", ["dominant", "edge_zeros", "staircase"])
def test_weight_geometry(dev, case, N):
    """One weight of 2^41 - N + 1 among ones, at the median rank; zero weights
    on the 50 smallest and the 50 largest points; weights whose fixed-point
    truncation piles up below the knots (oracle.quantile_exact.dyadic_weights)."""
    pts, w, m = qe.dyadic_case(case, N)
    ref = qe.ExactQuantile(pts, m)
    if case == "dominant":
        check(case, N, pts, w, ref, qe.dominant_alphas(ref, m), decided=True)
    elif case == "staircase":
        check(case, N, pts, w, ref, qe.staircase_alphas(ref), decided=True)
    else:
        # np.interp's rules: xp_0 .. xp_49 = 0 = alpha takes the last of the
        # equal knots (a zero-weight point); alpha = 1 = xp_{N-1} the largest
        assert ref(0.0).q == ref.p[49] and ref(1.0).q == ref.p[-1]
        assert not ref(0.0).clamp and not ref(1.0).clamp
        check(case, N, pts, w, ref, qe.alpha_set(ref), decided=True)


@pytest.mark.parametrize("N", [N_ONE, N_FOUR])
def test_unnormalised_ones(dev, N):
    """QuantileEpsilon(weighted=False): torch.ones(N) against the exact
    reference with total N (xp = (j + 1/2) / N rounds once: general rule)."""
    pts = qe.points_recipe(qe.seed(f"ones:{N}"), N, "normal")
    w = np.ones(N)
    ref = qe.ExactQuantile(pts, w)
    check("ones", N, pts, w, ref, qe.alpha_set(ref), dyadic=False, decided=True)


@pytest.mark.parametrize("N", [N_ONE, N_FOUR])
def test_power_of_two_scaling(dev, N):
    """Dyadic weights times 2^-600 and 2^+600: the same bits as unscaled, on
    both kernels."""
    pts, w, m = qe.dyadic_case("normal", N)
    ref = qe.ExactQuantile(pts, m)
    alphas = qe.alpha_set(ref)
    base, _ = check("scale", N, pts, w, ref, alphas, decided=True)
    P = T(pts)
    base_s = run(P, T(w), alphas, sorted_path=True)
    for e in (-600, 600):
        W = T(np.ldexp(w, e))
        assert run(P, W, alphas).tobytes() == base.tobytes(), e
        assert run(P, W, alphas, sorted_path=True).tobytes() == base_s.tobytes(), e


@pytest.mark.parametrize("N", [N_ONE, N_FOUR])
@pytest.mark.parametrize("case", list(qe.GENERAL_CASES))
def test_general_weights(dev, case, N):
    """uniform(0.5, 1.5) and exp(6 z) weights normalised by numpy, on
    continuous points and on two clusters (alpha on the gap's midpoint, where
    the slope is ~N times the gap)."""
    pts, w = qe.general_case(case, N)
    ref = qe.ExactQuantile(pts, w)
    alphas = qe.alpha_set(ref, exact_knots=False)
    if case.startswith("two_cluster"):
        g = int(np.searchsorted(ref.p, 500.0))
        alphas.append((ref.knot(g - 1) + ref.knot(g)) / 2)
    # the clusters are "crowded" data (the segment keeps its far neighbour)
    # and exp(6 z) leaves most fixed-point weights 0: those may go to the
    # sorted kernel
    check(case, N, pts, w, ref, alphas, dyadic=False, decided=(case == "uniform"))
    for key in sorted(SHARE):
        print(f"share of the general budget used: {key} {SHARE[key]:.3e}")


@pytest.mark.parametrize("N", [1000, N_ONE, N_FOUR])
def test_all_zero_weights(dev, N):
    """No positive weight: xp = 0 / 0 has no knots.  Both kernels write NaN,
    and the rerun of resolve_quantile ends there."""
    from pyabc_amd import gpu
    pts = qe.points_recipe(qe.seed(f"zero:{N}"), N, "normal")
    P, W = T(pts), T(np.zeros(N))
    for a in (0.0, 0.3, 1.0):
        raw = float(gpu.weighted_quantile(P, W, a).cpu()[0])
        srt = float(gpu.weighted_quantile(P, W, a, sorted_path=True).cpu()[0])
        assert np.isnan(raw) and np.isnan(srt), (N, a, raw, srt)
        assert np.isnan(gpu.resolve_quantile(raw, P, W, a))
        assert np.isnan(qe.weighted_quantile_exact(pts, np.zeros(N), a).q)
    # the next call on the shared workspace is not disturbed
    w, m, _ = qe.dyadic_weights(qe.seed(f"zero-after:{N}"), N, "flat")
    ref = qe.ExactQuantile(pts, m)
    check("after_zero", N, pts, w, ref, [0.5], decided=True)


# ---- e. calls as a sequence --------------------------------------------------------------

CTL_BYTES = 256 + 25 * 256     # WqCtl (56 bytes, its 256-byte slot) + the hs lines

SEQUENCE = [(N_FOUR, "normal"), (3, "normal"), (4097, "normal"), (200_003, "discrete"),
            (N_ONE, "normal"), (N_FOUR, "heavy_ties"), (1, "normal"), (1 << 20, "normal"),
            (32_769, "normal")]


def test_call_sequence(dev):
    """One private zeroed workspace, one stream, every call queued before any
    result is read: both launch paths in turn, two calls that end undecided.
    Each result equals, bit for bit, the same call on its own zeroed
    workspace; afterwards the control block and the hs lines are zero; then
    the same in reverse order on the same buffer."""
    from pyabc_amd import gpu, _native as nat

    def call(P, W, ws):
        q = torch.empty(1, dtype=torch.float64, device=dev)
        nat.call("abc_weighted_quantile", gpu.p(P), gpu.p(W), P.numel(), 0.5, gpu.p(q),
                 gpu.p(ws), ws.numel(), gpu.stream_ptr())
        return q

    nbytes = max(nat.query("abc_weighted_quantile_workspace", n) for n, _ in SEQUENCE)
    inputs, alone = [], []
    for n, recipe in SEQUENCE:
        rng = qe.seed(f"seq:{recipe}:{n}")
        pts = qe.points_recipe(rng, n, recipe)
        w, m, _ = qe.dyadic_weights(rng, n, "flat")
        P, W = T(pts), T(w)
        inputs.append((P, W))
        q = call(P, W, torch.zeros(nbytes, dtype=torch.uint8, device=dev)).cpu().numpy()
        alone.append(q)
        undecided = recipe in ("discrete", "heavy_ties")
        assert np.isnan(q[0]) == undecided, (n, recipe, q)
        if not undecided:
            within(q[0], qe.ExactQuantile(pts, m)(0.5), n, True, ("select", recipe, n, 0.5))
    alone = np.concatenate(alone)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    for order in (range(len(SEQUENCE)), reversed(range(len(SEQUENCE)))):
        order = list(order)
        got = torch.cat([call(*inputs[i], ws) for i in order]).cpu().numpy()
        assert got.tobytes() == alone[order].tobytes(), (order, got, alone[order])
        assert not ws[:CTL_BYTES].cpu().numpy().any()


# ---- f. through the product ------------------------------------------------------------------

@pytest.mark.parametrize("N", [N_ONE, N_FOUR])
@pytest.mark.parametrize("weighted", [False, True])
def test_quantile_epsilon(dev, weighted, N):
    """QuantileEpsilon._update on a device (distance, weight) pair: alpha 0.3,
    with and without a multiplier; weighted=False replaces the weights by
    ones.  A discrete-distance input takes its value from the sorted rerun."""
    from pyabc_amd.epsilon import QuantileEpsilon
    pts, w, m = qe.dyadic_case("normal", N)
    disc = qe.points_recipe(qe.seed(f"eps-discrete:{N}"), N, "discrete")
    for d in (pts, disc):
        wd = types.SimpleNamespace(device_distance=T(d), device_w=T(w))
        r = qe.ExactQuantile(d, m if weighted else np.ones(N))(0.3)
        for mult in (1.0, 1.25):
            eps = QuantileEpsilon(alpha=0.3, quantile_multiplier=mult, weighted=weighted)
            eps._update(0, wd)
            pending = eps._look_up[0]
            raw = float(pending.q_dev.cpu()[0])
            assert np.isnan(raw) == (d is disc), (N, weighted, raw)
            v = eps(0)
            assert isinstance(v, float) and eps(0) == v
            if weighted:
                tol = qe.budget_dyadic(r)
            else:
                tol, _ = qe.budget_general(r, N)
            # q * multiplier rounds once more
            assert abs(v - r.q * mult) <= tol * mult + np.spacing(abs(v)), (N, weighted, mult,
                                                                            v, r)
