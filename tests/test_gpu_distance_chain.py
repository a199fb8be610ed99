"""The distance-and-accept chain against exact references
(oracle/distance_exact.py; inputs and bounds in tests/distance_chain_ref.py):

    abc_pnorm (row path S <= 32, wave path) -> abc_mask_gave_up
    -> abc_accept_compact, and the paths that must give the same bits or the
    same accepted positions: abc_pnorm_accept, abc_aggregate_distance,
    abc_aggregate_accept, PNormDistance.__call__; and abc_sort_pairs_f64 past
    its single-block scan (the sorted quantile feeds eps from these distances).

float64 numpy is a peer of these kernels; the reference here is exact (integer
sums, mpmath roots) and the comparison is against the exact value, not its
rounding.  u = 2^-53.  Every bound is derived from the kernels' code:

    term   a_k = |fl(wf_k fl(x_k - x0_k))|: two roundings, 2 u
    p = inf  the max of the a_k: 2 u
    p = 1    S - 1 additions of non-negative partial sums (row path: in k
             order; wave path: ceil(S / 64) - 1 per lane and 6 tree levels,
             fewer), u each: (S + 1) u, asserted as the issue's (S + 2) u
    p = 2    a_k^2 carries 4 u and its own rounding, the sum S - 1 more, the
             square root halves that and rounds once: ((S + 4) / 2 + 1) u to
             first order.  The issue sets ((S + 3) / 2 + 1) u, half a u less;
             that is what is asserted (either is reached only if every
             rounding of a row points the same way)
    any p    a_k^p carries 2 p u and pow's K_pow ulps (1 ulp <= 2 u), the sum
             S - 1 more; pow(s, fl(1 / p)) divides that by p, adds K_pow ulps
             and, because 1 / p is itself rounded (relative u), a factor
             s^(u / p): |ln s| u / p.  In all
                 ((2 p + 2 K_pow + S - 1) / p + |ln s| / p + 2 K_pow) u
             with s = sum_k |term_k|^p from the oracle.  K_pow:
             distance_chain_ref.K_POW.

Each case prints ``DIST <what> max err / bound = <largest>``.

The fused candidate round (sim_pnorm / pnorm_acc / pnorm_finish) simulates its
own statistics from finite parameters, so the API cannot hand it a NaN
statistic; its p = inf accumulation takes the same NaN-keeping max and is held
by test_fused_pnorm_orders and test_fused_equals_staged staying bit-equal to
the staged kernels tested here.
"""
import math

import numpy as np
import pytest

import distance_chain_ref as ref
from oracle import distance_exact as dx

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U = ref.U
INF, NAN = math.inf, math.nan


@pytest.fixture(scope="module")
def dev():
    from pyabc_amd import gpu
    return gpu.require_device()


def T(a, dtype=None):
    from pyabc_amd import gpu
    return gpu.as_dev(a, dtype=dtype)


def pname(p):
    return "inf" if p == INF else f"{p:g}"


def check_against_exact(got, r, S, p, what, exact_bits=False):
    """got [B] against the PNormExact r (its first B rows): NaN and +inf rows
    and exact zeros as bit patterns, the rest within bound_u; -> the largest
    err / bound."""
    B = len(got)
    r = dx.PNormExact(*(np.asarray(f)[:B] for f in r))
    e, ok = ref.rel_err_u(got, r)
    np.testing.assert_array_equal(ref.bits(got[~ok]), ref.bits(r.d[~ok]),
                                  err_msg=f"{what}: special / zero rows")
    if exact_bits:
        np.testing.assert_array_equal(ref.bits(got), ref.bits(r.d), err_msg=what)
    if not ok.any():
        return 0.0
    bound = ref.bound_u(S, p, r.sum_p)
    ratio = np.abs(e) / bound
    worst = float(ratio[ok].max())
    assert worst <= 1.0, (what, int(np.argmax(np.where(ok, ratio, 0))), worst)
    return worst


# ---- abc_pnorm against the exact oracle ------------------------------------------------

@pytest.mark.parametrize("p", ref.P_LIST, ids=pname)
@pytest.mark.parametrize("S", ref.S_LIST)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_pnorm_exact(dev, family, S, p):
    """Every B of B_LIST (the row path's 256-thread blocks; the wave path's 8
    rows per wave and 4 waves per block, ragged) at every S (the row / wave
    switch at 32, the lane stride at 64) within the bound of the module
    docstring; small integers under p in {1, 2, inf} to the bit (exact sums
    below 2^53 and a correctly rounded sqrt)."""
    from pyabc_amd import gpu
    x, x0, wf = ref.inputs(family, S)
    r = ref.reference(family, S, p)
    assert (r.kind == dx.FINITE).all()
    xd, x0d, wfd = T(x), T(x0), T(wf)
    worst = 0.0
    for B in ref.B_LIST:
        got = gpu.pnorm(xd[:B], x0d, wfd, p).cpu().numpy()
        worst = max(worst, check_against_exact(
            got, r, S, p, f"{family} S={S} B={B} p={pname(p)}",
            exact_bits=(family == "integers" and p in (1.0, 2.0, INF))))
    print(f"DIST pnorm {family} S={S} p={pname(p)} max err / bound = {worst:.3f}")


# ---- special values -----------------------------------------------------------------------

def special_matrices(S):
    for kind in ref.SPECIAL_KINDS:
        for col in ref.special_columns(S):
            yield kind, col, ref.special_case(kind, S, col)


@pytest.mark.parametrize("p", ref.P_LIST, ids=pname)
@pytest.mark.parametrize("S", ref.SPECIAL_S)
def test_pnorm_special_values(dev, S, p):
    """NaN, +-inf, inf - inf, 0 inf, a NaN observation and -0.0 differences in
    the first, a middle and the last column (and column 64 of wide rows) of
    the first, a middle and the last row: the oracle's table as bit patterns
    (NaN rows NaN for EVERY p -- p = inf's max must not drop it -- infinite
    rows +inf, all-zero rows +0.0), the untouched rows within the bound."""
    from pyabc_amd import gpu
    n_nan = 0
    for kind, col, (x, x0, wf) in special_matrices(S):
        r = dx.pnorm_exact(x, x0, wf, p)
        got = gpu.pnorm(T(x), T(x0), T(wf), p).cpu().numpy()
        check_against_exact(got, r, S, p, f"{kind} S={S} col={col} p={pname(p)}",
                            exact_bits=p in (1.0, 2.0, INF))
        n_nan += int((r.kind == dx.NAN).sum())
        if kind == "neg_zero":
            assert ref.bits(got[:1])[0] == 0, "all-zero row is +0.0"
    assert n_nan >= 3 * 5 * len(ref.special_columns(S))


def test_pnorm_fp64_edges(dev):
    """The format's edges, pinned as they are: the kernels square in float64.
    One |term| = 1e200 under p = 2 overflows to +inf (numpy's result too; the
    exact distance is 1e200) and is accepted at eps = inf only; terms <=
    1e-170 square to 0 and the distance is 0 (exact: ~1e-170)."""
    from pyabc_amd import gpu
    for S in (5, 33):
        x = np.ones((3, S))
        x[1, S - 1] = 1e200
        x[2, :] = 1e-170 * np.arange(1, S + 1) / S
        d = gpu.pnorm(T(x), T(np.zeros(S)), T(np.ones(S)), 2.0)
        got = d.cpu().numpy()
        assert got[0] == math.sqrt(S) and got[1] == INF and ref.bits(got[2:])[0] == 0
        for eps, want in ((1e308, [0, 2]), (INF, [0, 1, 2])):
            idx, cnt = gpu.accept_compact(d, eps)
            assert idx.cpu().numpy()[:int(cnt.cpu())].tolist() == want
        r = dx.pnorm_exact(x, np.zeros(S), np.ones(S), 2.0)
        assert r.d[1] == 1e200 and 0 < r.d[2] <= 1e-169


# ---- every path equals abc_pnorm -------------------------------------------------------------

def staged_accept(d, eps):
    """abc_pnorm's distances through abc_accept_compact -> positions."""
    from pyabc_amd import gpu
    idx, cnt = gpu.accept_compact(d, eps)
    return idx.cpu().numpy()[:int(cnt.cpu())]


def run_accept(fn, *args):
    idx, cnt = fn(*args)
    return idx.cpu().numpy()[:int(cnt.cpu())]


def chain_matrices(S):
    """The special-value matrices and benign rows (B = 257: two blocks of the
    row path, a ragged last wave of the wave path) with an exact-tie eps."""
    for kind, col, m in special_matrices(S):
        yield f"{kind}@{col}", m, None
    x, x0, wf = ref.inputs("benign", S, 257)
    yield "benign", (x, x0, wf), 100


@pytest.mark.parametrize("S", ref.SPECIAL_S)
def test_every_path_equals_pnorm(dev, S):
    """abc_pnorm_accept, abc_aggregate_distance (K = 1; K = 3 on the SIMPLE
    kernels, p in {1, 2, inf}, and on the general ones), abc_aggregate_accept
    and PNormDistance.__call__ give abc_pnorm's bits or the accepted positions
    of abc_pnorm + abc_mask_gave_up + abc_accept_compact; abc_pnorm itself is
    held to the oracle above, so agreement here is agreement with the oracle.
    eps: one row's own distance (an exact tie) and inf.  No row the oracle
    makes NaN is ever accepted."""
    from pyabc_amd import gpu
    from pyabc_amd.distance import PNormDistance
    rng = np.random.default_rng(S)
    keys = [f"s{k:03d}" for k in range(S)]
    for name, (x, x0, wf), tie_row in chain_matrices(S):
        B = len(x)
        xd, x0d = T(x), T(x0)
        gave_up = np.arange(B) % 5 == 2          # (none of the special rows)
        att = torch.as_tensor(np.where(gave_up, 11, 10), dtype=torch.int32, device=xd.device)
        w3 = np.stack([wf, wf * rng.uniform(0.5, 2.0, S), wf[::-1].copy()])
        c3 = np.array([0.7, 1.3, 2.1])
        per_p = {}
        for p in ref.P_LIST:
            msg = f"{name} S={S} p={pname(p)}"
            kind = dx.classify(x, x0, wf)
            d = gpu.pnorm(xd, x0d, T(wf), p)
            dn = d.cpu().numpy()
            per_p[p] = dn
            assert np.array_equal(np.isnan(dn), kind == dx.NAN), msg
            # K = 1, c = 1: 0 + 1 t = t
            st1 = gpu.TermStack(T(wf[None, :]), [p], [1.0])
            out, tm = gpu.aggregate_distance(xd, x0d, st1, terms=True)
            np.testing.assert_array_equal(ref.bits(tm.cpu().numpy()[:, 0]), ref.bits(dn), msg)
            np.testing.assert_array_equal(ref.bits(out.cpu().numpy()), ref.bits(dn), msg)
            # PNormDistance.__call__ on single rows: the special ones and two others
            dist = PNormDistance(p=p, weights=dict(zip(keys, wf)))
            for b in sorted({0, B // 2, B - 1, 1, B - 2} & set(range(B))):
                one = dist(dict(zip(keys, x[b])), dict(zip(keys, x0)), t=0)
                assert ref.bits(np.array([one]))[0] == ref.bits(dn[b:b + 1])[0], (msg, b)
            fin = dn[np.isfinite(dn)]
            ties = [float(dn[tie_row])] if tie_row is not None else \
                ([float(np.sort(fin)[len(fin) // 2])] if len(fin) else [])
            dm = gpu.mask_gave_up(d.clone(), att, 10)
            for eps in ties + [INF]:
                want = staged_accept(dm, eps)
                np.testing.assert_array_equal(
                    want, dx.accept_exact(np.where(gave_up, NAN, dn), eps), msg)
                assert not (kind[want] == dx.NAN).any(), msg
                if eps != INF:
                    assert len(want) >= 1 or gave_up[dn == eps].all(), msg
                np.testing.assert_array_equal(
                    run_accept(gpu.pnorm_accept, xd, x0d, T(wf), p, eps, B, att, 10), want, msg)
                np.testing.assert_array_equal(
                    run_accept(gpu.aggregate_accept, xd, x0d, st1, eps, B, att, 10), want, msg)
        # K = 3, mixed p: every term is abc_pnorm's for its own weights and p
        for ps in ([1.0, 2.0, INF], [1.5, INF, 3.0]):
            st = gpu.TermStack(T(w3), ps, c3)
            out, tm = gpu.aggregate_distance(xd, x0d, st, terms=True)
            tmn, outn = tm.cpu().numpy(), out.cpu().numpy()
            for k in range(3):
                tk = per_p[ps[k]] if k == 0 else \
                    gpu.pnorm(xd, x0d, T(w3[k]), ps[k]).cpu().numpy()
                np.testing.assert_array_equal(ref.bits(tmn[:, k]), ref.bits(tk),
                                              f"{name} S={S} term {k} of {ps}")
            # a NaN term makes the row NaN (c NaN = NaN)
            row_nan = np.isnan(tmn).any(1)
            assert np.array_equal(np.isnan(outn), row_nan)
            kind3 = np.maximum.reduce([dx.classify(x, x0, w3[k]) for k in range(3)])
            assert np.array_equal(row_nan, kind3 == dx.NAN)
            fin = outn[np.isfinite(outn)]
            for eps in ([float(np.sort(fin)[len(fin) // 2])] if len(fin) else []) + [INF]:
                dm = gpu.mask_gave_up(out.clone(), att, 10)
                want = staged_accept(dm, eps)
                assert not row_nan[want].any()
                np.testing.assert_array_equal(
                    run_accept(gpu.aggregate_accept, xd, x0d, st, eps, B, att, 10), want,
                    f"{name} S={S} aggregate_accept {ps}")


# ---- decisions against the exact distance ------------------------------------------------------

DECISION_S = [2, 32, 33, 129]      # test_oracle_distance_exact checks the 1 % on these


@pytest.mark.parametrize("p", ref.P_LIST, ids=pname)
@pytest.mark.parametrize("family", ["benign", "wide"])
def test_decisions_against_exact(dev, family, p):
    """eps = the exact median distance (one row's own, B = 1037 is odd).  Every
    row farther from eps than the kernels' bound is accepted exactly when its
    exact distance is <= eps, by the staged chain and by the accept tail; the
    rows that close (the undecidable set, at most 1 %: checked on the oracle
    alone in tests/test_oracle_distance_exact.py) may go either way."""
    from pyabc_amd import gpu
    for S in DECISION_S:
        x, x0, wf = ref.inputs(family, S)
        r = ref.reference(family, S, p)
        eps = float(np.median(r.d))
        und = dx.undecidable(r, eps, ref.bound_u(S, p, r.sum_p) * U)
        assert und.sum() <= 0.01 * len(r.d)
        want = dx.accepted_exact(r, eps)
        xd, x0d, wfd = T(x), T(x0), T(wf)
        acc = np.zeros(len(x), dtype=bool)
        acc[staged_accept(gpu.pnorm(xd, x0d, wfd, p), eps)] = True
        tail = np.zeros(len(x), dtype=bool)
        tail[run_accept(gpu.pnorm_accept, xd, x0d, wfd, p, eps, len(x))] = True
        assert np.array_equal(acc[~und], want[~und]), (S, np.flatnonzero(acc != want))
        assert np.array_equal(tail, acc)
        print(f"DIST decisions {family} S={S} p={pname(p)} undecidable={int(und.sum())} "
              f"accepted={int(acc.sum())}/{len(x)}")


# ---- abc_accept_compact and abc_mask_gave_up edges ------------------------------------------------

COMPACT_B = [1, 2047, 2048, 2049, 524_288, 524_289, 1_050_000]
CT_TILE, CT_T = 2048, 256          # abc_sampler.hip


def compact_checked(dd, eps, what):
    """Positions ascending and equal to np.flatnonzero(d <= eps), the count
    exact, two runs the same bits."""
    from pyabc_amd import gpu
    d = T(dd)
    want = dx.accept_exact(dd, eps)
    runs = []
    for _ in range(2):
        idx, cnt = gpu.accept_compact(d, eps)
        n = int(cnt.cpu())
        assert n == len(want), (what, n, len(want))
        runs.append(idx.cpu().numpy()[:n])
    np.testing.assert_array_equal(runs[0], want, err_msg=what)
    assert runs[0].tobytes() == runs[1].tobytes(), what
    return want


@pytest.mark.parametrize("B", COMPACT_B)
def test_accept_compact_edges(dev, B):
    """B around one tile (2048) and where accept_scan_kernel's 256 threads
    own 1, 2 and 3 tiles each (B = 524 288: 256 tiles; 524 289: 257;
    1 050 000: 513).  Distances from {NaN, -0.0, 0.0, 5e-324, 1, inf} and
    random values against eps in {-1, -0.0, 0.0, a tie, inf, NaN}; nothing and
    everything accepted; accepted rows only in the last (partial) tile; only
    in the tiles of the last scan thread that owns any."""
    rng = np.random.default_rng(B)
    pool = np.array([NAN, -0.0, 0.0, 5e-324, 1.0, INF])
    dd = np.where(rng.uniform(size=B) < 0.5, pool[rng.integers(0, len(pool), B)],
                  rng.uniform(0.0, 2.0, B))
    tie = float(dd[B // 2]) if np.isfinite(dd[B // 2]) else 1.0
    for eps in (-1.0, -0.0, 0.0, 5e-324, tie, 1.0, INF, NAN):
        got = compact_checked(dd, eps, f"B={B} eps={eps}")
        if eps == -1.0 or eps != eps:
            assert len(got) == 0
    # everything accepted
    allin = rng.uniform(0.0, 2.0, B)
    assert len(compact_checked(allin, INF, f"B={B} all")) == B
    assert len(compact_checked(allin, 2.0, f"B={B} all <= 2")) == B
    # only the last tile (partial unless B is a multiple of the tile)
    nt = -(-B // CT_TILE)
    last = np.full(B, 2.0)
    last[(nt - 1) * CT_TILE:] = 0.5
    last[B - 1] = 1.0                                    # the tie, in the last slot
    got = compact_checked(last, 1.0, f"B={B} last tile")
    assert len(got) == B - (nt - 1) * CT_TILE and got[-1] == B - 1
    # only the tiles of the last scan thread that owns any
    per = -(-nt // CT_T)
    first_tile = ((nt - 1) // per) * per
    own = np.full(B, NAN)
    own[first_tile * CT_TILE:] = rng.uniform(0.0, 1.0, B - first_tile * CT_TILE)
    got = compact_checked(own, 0.5, f"B={B} last scan thread")
    assert len(got) == 0 or got[0] >= first_tile * CT_TILE


def test_mask_gave_up_edges(dev):
    """att == max_attempts is kept, att == max_attempts + 1 masked; the
    default value (NaN) keeps a gave-up row out at eps = inf; a caller's value
    is written as given."""
    from pyabc_amd import gpu
    for B in (1, 255, 256, 257, 2049):
        rng = np.random.default_rng(B)
        dd = rng.uniform(size=B)
        att_h = rng.choice(np.array([1, 9, 10, 11, 12, 32767], dtype=np.int32), B)
        att = torch.as_tensor(att_h, device="cuda")
        d = gpu.mask_gave_up(T(dd), att, 10)
        got = d.cpu().numpy()
        kept = att_h <= 10
        np.testing.assert_array_equal(ref.bits(got), ref.bits(np.where(kept, dd, NAN)))
        np.testing.assert_array_equal(staged_accept(d, INF), np.flatnonzero(kept))
        np.testing.assert_array_equal(staged_accept(d, 0.5), np.flatnonzero(kept & (dd <= 0.5)))
        d2 = gpu.mask_gave_up(T(dd), att, 10, value=-INF).cpu().numpy()
        np.testing.assert_array_equal(ref.bits(d2), ref.bits(np.where(kept, dd, -INF)))


# ---- abc_sort_pairs_f64 past the single-block scan ---------------------------------------------------

@pytest.mark.parametrize("N", [131_072, 131_073, 140_001])
def test_sort_pairs_past_single_scan(dev, N):
    """run_sort scans its 256 x ceil(N / 2048) histogram in one block up to
    16384 entries (N <= 131 072) and with three kernels beyond.  Keys with
    heavy ties, +-0.0, +-inf and NaN against np.argsort(kind="stable"): the
    values are the permutation, the keys its bit patterns.  Two things are
    the key map's and are left as they are: -0.0 ties with +0.0 (numpy's
    comparison too) and comes back as +0.0, so the expected keys are k + 0.0;
    NaN is ordered by its sign bit -- np.nan (positive) sorts last, as in
    numpy, and only that NaN is fed."""
    from pyabc_amd import gpu
    rng = np.random.default_rng(N)
    k = rng.integers(0, 10, N).astype(np.float64)               # ties by the thousand
    u = rng.uniform(size=N)
    k = np.where(u < 0.2, rng.standard_normal(N) * 10 ** rng.uniform(-300, 300, N), k)
    pool = np.array([0.0, -0.0, INF, -INF, np.nan])
    sp = u > 0.9
    k[sp] = pool[rng.integers(0, len(pool), int(sp.sum()))]
    k[[0, N // 2, N - 1]] = [np.nan, -INF, -0.0]
    v = np.arange(N, dtype=np.float64)
    ko, vo = gpu.sort_pairs(T(k), T(v))
    order = np.argsort(k, kind="stable")
    np.testing.assert_array_equal(vo.cpu().numpy(), v[order])
    np.testing.assert_array_equal(ref.bits(ko.cpu().numpy()), ref.bits((k + 0.0)[order]))
