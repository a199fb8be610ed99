"""Every workspace-taking entry stays inside the bytes its query returns.

Each case runs a gpu.py wrapper twice: once as it is, and once with
gpu.workspace handing out a private zeroed buffer of exactly the query's
bytes followed by a 4096-byte guard pattern.  The guard must survive and the
outputs must agree bit for bit.  The recorded C call is then repeated with
ws_bytes one short: ABC_ERR_WORKSPACE, and pre-filled outputs untouched.
Every call is a valid call inside its own allocation."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD, PATTERN, SENTINEL = 4096, 0xA5, 0x5C
KN_MIN_N = 2048     # abc_local_knn.h: the k-NN select starts here


@pytest.fixture(scope="module")
def dev():
    from pyabc_amd import gpu
    return gpu.require_device()


def T(a, dtype=None):
    from pyabc_amd import gpu
    return gpu.as_dev(a, dtype=dtype)


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def check_entry(monkeypatch, entry, fn):
    """fn() calls `entry` once through gpu.py and returns its output tensors."""
    from pyabc_amd import _native as nat
    from pyabc_amd import gpu
    ref = [t.clone() for t in fn()]
    bufs, calls = [], []

    def private_ws(nbytes, slot="main"):
        n = int(nbytes)
        buf = torch.zeros(n + GUARD, dtype=torch.uint8, device="cuda")
        buf[n:] = PATTERN
        bufs.append((buf, n))
        return buf[:n]

    real_call = nat.call

    def recording_call(name, *args):
        if name == entry:
            calls.append(args)
        return real_call(name, *args)

    with monkeypatch.context() as m:
        m.setattr(gpu, "workspace", private_ws)
        m.setattr(nat, "call", recording_call)
        got = fn()
    torch.cuda.synchronize()
    assert len(calls) == 1 and len(bufs) == 1, (entry, len(calls), len(bufs))
    buf, n = bufs[0]
    assert bool((buf[n:] == PATTERN).all()), f"{entry}: guard overwritten"
    assert len(ref) == len(got)
    for k, (a, b) in enumerate(zip(ref, got)):
        assert torch.equal(_bits(a), _bits(b)), f"{entry}: output {k} differs"

    # one byte short: refused before anything is written
    args = list(calls[0])
    i = args.index(buf.data_ptr())
    assert args[i + 1] == n
    args[i + 1] = n - 1
    for t in got:
        _bits(t).fill_(SENTINEL)
    with pytest.raises(nat.NativeError) as ei:
        real_call(entry, *args)
    assert ei.value.code == nat.ABC_ERR_WORKSPACE
    assert "workspace" in nat.load().abc_last_error().decode()
    torch.cuda.synchronize()
    for k, t in enumerate(got):
        assert bool((_bits(t) == SENTINEL).all()), f"{entry}: output {k} written"
    assert bool((buf[n:] == PATTERN).all())


# ---- reductions, compaction, sort, quantile ------------------------------------

def _weights(rng, n):
    w = np.exp(0.5 * rng.standard_normal(n))
    return w / w.sum()


@pytest.mark.parametrize("N,d", [(3000, 10), (300, 80)])
def test_moments(dev, monkeypatch, N, d):
    from pyabc_amd import gpu
    rng = np.random.default_rng(1)
    X, w = T(rng.standard_normal((N, d))), T(_weights(rng, N))
    check_entry(monkeypatch, "abc_weighted_moments",
                lambda: (gpu.weighted_moments_dev(X, w),))


def test_scan_normalize_compact(dev, monkeypatch):
    from pyabc_amd import gpu
    rng = np.random.default_rng(2)
    n = 5001
    w = T(_weights(rng, n))
    check_entry(monkeypatch, "abc_inclusive_scan_f64", lambda: (gpu.inclusive_scan(w),))

    def normalize():
        v = (3.0 * w).clone()
        return v, gpu.normalize_weights(v)
    check_entry(monkeypatch, "abc_normalize_weights", normalize)
    dist = T(rng.random(n))
    check_entry(monkeypatch, "abc_accept_compact", lambda: gpu.accept_compact(dist, 0.5))


@pytest.mark.parametrize("N", [1, 70_001])
def test_sort(dev, monkeypatch, N):
    from pyabc_amd import gpu
    rng = np.random.default_rng(3)
    k, v = T(rng.standard_normal(N)), T(rng.random(N))
    check_entry(monkeypatch, "abc_sort_pairs_f64", lambda: gpu.sort_pairs(k, v))


@pytest.mark.parametrize("N", [1000, (1 << 20) + 1])   # one launch | four launches
def test_quantile(dev, monkeypatch, N):
    from pyabc_amd import gpu
    rng = np.random.default_rng(4)
    pts, w = T(rng.standard_normal(N)), T(_weights(rng, N))
    check_entry(monkeypatch, "abc_weighted_quantile",
                lambda: (gpu.weighted_quantile(pts, w, 0.3),))


def test_quantile_sorted(dev, monkeypatch):
    from pyabc_amd import gpu
    rng = np.random.default_rng(5)
    N = 1000
    pts, w = T(rng.standard_normal(N)), T(_weights(rng, N))
    check_entry(monkeypatch, "abc_weighted_quantile_sorted",
                lambda: (gpu.weighted_quantile(pts, w, 0.3, sorted_path=True),))


# ---- column statistics ---------------------------------------------------------

# R = 100: the std layout is the larger one; R = 4097: the select's
@pytest.mark.parametrize("R,S", [(100, 12), (4097, 3)])
def test_column_stats(dev, monkeypatch, R, S):
    from pyabc_amd import gpu
    rng = np.random.default_rng(6)
    X = T(rng.standard_normal((R, S)))
    check_entry(monkeypatch, "abc_column_std", lambda: (gpu.column_std(X),))
    check_entry(monkeypatch, "abc_column_mad", lambda: (gpu.column_mad(X),))


@pytest.mark.parametrize("kind", range(10))
def test_column_scale(dev, monkeypatch, kind):
    from pyabc_amd import gpu
    rng = np.random.default_rng(7)
    R, S = 4097, 3
    X, x0 = T(rng.standard_normal((R, S))), T(rng.standard_normal(S))
    check_entry(monkeypatch, "abc_column_scale", lambda: (gpu.column_scale(X, kind, x0),))


# ---- mvn density ---------------------------------------------------------------

@pytest.fixture(scope="module")
def mvn_case(dev):
    rng = np.random.default_rng(8)
    N = M = 4096
    d = 10
    X = 0.8 + np.sqrt(0.2) * rng.standard_normal((N, d))
    w = _weights(rng, N)
    return X, w, M


@pytest.mark.parametrize("prec,hinted", [("f64", False), ("f32", False),
                                         ("x3", False), ("x3", True)])
def test_mvn_logpdf(dev, monkeypatch, mvn_case, prec, hinted):
    import pandas as pd
    from pyabc_amd.transition import MultivariateNormalTransition
    X, w, M = mvn_case
    N, d = X.shape
    t = MultivariateNormalTransition(precision=prec)
    t.fit(pd.DataFrame(X, columns=[f"p{k}" for k in range(d)]), w.copy())
    th, _, anc, _ = t.propose_device(M)
    hint = None
    if hinted:
        # the ancestors, but a far row and an invalid one now and then: a few
        # candidates take the nested exact pass
        far = int(np.argmax(((X - X.mean(0)) ** 2).sum(1)))
        h = anc.cpu().numpy().copy()
        h[::500] = far
        h[::700] = -1
        hint = T(h, dtype=torch.int64)
    check_entry(monkeypatch, "abc_mvn_logpdf", lambda: (t.logpdf_device(th, hint=hint),))


# ---- LocalTransition -------------------------------------------------------------

FIT_CASES = [
    (KN_MIN_N - 1, 5, 200),        # dense moments, no k-NN select (k > N / 16)
    (KN_MIN_N + 1, 3, 10),         # k-NN select, list mode
    (KN_MIN_N + 1, 12, 10),        # k-NN select, no list
    (KN_MIN_N + 1, 5, (KN_MIN_N + 1) // 4),   # deferred collect
    (300, 20, 10),                 # wide kernel, matrices in LDS
    (300, 80, 10),                 # wide kernel, matrices in the workspace
]


@pytest.mark.parametrize("N,d,k", FIT_CASES)
def test_local_fit(dev, monkeypatch, N, d, k):
    from pyabc_amd import gpu
    rng = np.random.default_rng(9)
    X, w = T(rng.standard_normal((N, d))), T(_weights(rng, N))
    check_entry(monkeypatch, "abc_local_fit", lambda: gpu.local_fit(X, w, k, 1.0, 1e-3))


@pytest.mark.parametrize("d", [5, 12])
def test_local_logpdf(dev, monkeypatch, d):
    from pyabc_amd import gpu
    rng = np.random.default_rng(10)
    N, M = 2049, 1000
    X, w = T(rng.standard_normal((N, d))), T(_weights(rng, N))
    _, inv, _, _, lnorm = gpu.local_fit(X, w, 50, 1.0, 1e-3)
    x = T(rng.standard_normal((M, d)))
    check_entry(monkeypatch, "abc_local_logpdf",
                lambda: (gpu.local_logpdf(x, X, w, inv, lnorm),))


# ---- candidate rounds --------------------------------------------------------------

def test_candidates(dev, monkeypatch):
    from pyabc_amd import gpu
    rng = np.random.default_rng(11)
    N, d, B = 3000, 10, 4097
    X, w = T(0.3 + rng.standard_normal((N, d))), T(_weights(rng, N))
    cdf = gpu.inclusive_scan(w)
    L = T(np.linalg.cholesky(0.2 * np.eye(d) + 0.05))
    kinds = torch.zeros(d, dtype=torch.int32, device=dev)
    params = T(np.tile([0.0, 1.0, 0.0, 0.0], d))
    src = torch.arange(d, dtype=torch.int32, device=dev)
    ones = T(np.ones(d))
    rnd = gpu.CandidateRound(d, d, kinds, params, src, ones, T(np.full(d, 0.5)),
                             T(np.full(d, 0.3)), ones, 2.0, 11, 1, 100, X=X, cdf=cdf,
                             guide=gpu.cdf_guide(cdf), L=L)

    def full(idx, cnt):
        idx[int(cnt.item()):] = -1   # positions past the count are not written
        return idx, cnt
    check_entry(monkeypatch, "abc_candidates_round",
                lambda: full(*rnd.run(0, B, 3.0, B)))
    check_entry(monkeypatch, "abc_candidates_propose", lambda: rnd.propose(0, B))
    x = T(rng.standard_normal((B, d)))
    check_entry(monkeypatch, "abc_pnorm_accept",
                lambda: full(*gpu.pnorm_accept(x, ones, ones, 2.0, 3.0, B)))


# ---- bootstrap cv, temperature sums ---------------------------------------------------

def test_bootstrap_cv_and_temper(dev, monkeypatch):
    from pyabc_amd import _native as nat
    from pyabc_amd import gpu
    rng = np.random.default_rng(12)
    ld, w = T(rng.standard_normal((20, 3001))), T(_weights(rng, 3001))
    check_entry(monkeypatch, "abc_bootstrap_cv", lambda: gpu.bootstrap_cv(ld, w))
    R = 5001
    dens, lr = T(-rng.random(R)), T(rng.standard_normal(R))

    def temper():   # gpu.temper_sums' call, its result left on the device
        out = torch.empty(2, dtype=torch.float64, device=dev)
        ws = gpu.workspace(nat.query("abc_temper_workspace"), "temper")
        nat.call("abc_temper_sums", gpu.p(dens), gpu.p(lr), None, R, 0.0, 1,
                 gpu.TEMPER_ACCEPTANCE, 0.3, 0.0, gpu.p(out), gpu.p(ws), ws.numel(),
                 gpu.stream_ptr())
        return (out,)
    check_entry(monkeypatch, "abc_temper_sums", temper)
