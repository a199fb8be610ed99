"""The x3 density kernel's pass-2 loop at the population sizes where its
structure changes (d = 10, so mvn_x3_kernel<5, 6, *> runs).

For small N the plan is 8 chunks of ceil(NT / 8) 32-row tiles, and a chunk runs
groups of four tiles, then a tile pair, then an odd tile:

    N          tiles per chunk   what it checks
    1, 31, 33  1                 one or two tiles, partial rows; chunks past the
                                 end load nothing
    256        1                 only the peeled odd tile
    512        2                 one full pair, no tail
    768        3                 one pair plus the odd tile
    1280       5                 a flush after 4 tiles, then a tail
    539        3 (NT = 17)       chunk 5 has 2 tiles, chunks 6 and 7 are empty
    2304       9                 two flushes plus an odd tail

against M in {1, 191, 192, 193, 769} candidates: a wave's 6 tiles full and
partial, and a second block.  Reference: the fp64 oracle at 1e-6 relative in
density (the bar of test_gpu_rows.py::test_c3_density_full_population), with
the sampler's ancestor hints and without (the exact max pre-pass).
"""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D = 10
NS = [1, 31, 33, 256, 512, 768, 1280, 539, 2304]
MS = [1, 191, 192, 193, 769]
M_MAX = max(MS)


@pytest.fixture(scope="module")
def dev():
    from pyabc_amd import gpu
    return gpu.require_device()


_cases = {}


def _case(N, dev):
    """Fitted transition, 769 proposed candidates with their ancestors and the
    oracle's log densities for population size N (built once per N)."""
    if N not in _cases:
        import pyabc_amd as pa
        g = torch.Generator(device="cpu").manual_seed(1000 + N)
        X = 0.8 + 0.45 * torch.randn(N, D, generator=g, dtype=torch.float64)
        w = torch.exp(0.3 * torch.randn(N, generator=g, dtype=torch.float64))
        w /= w.sum()
        tr = pa.MultivariateNormalTransition()
        tr.fit_device(X.to(dev), w.to(dev), [f"p{k}" for k in range(D)])
        th, lp, anc, att = tr.propose_device(M_MAX, seed=3, generation=1, idx0=0)
        ref = oracle.mvn_logpdf(th.cpu().numpy(), X.numpy(), w.numpy(), tr.cov)
        assert np.isfinite(ref).all()
        _cases[N] = (tr, th, anc, ref)
    return _cases[N]


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", NS)
def test_x3_loop_shapes(dev, N, M):
    tr, th, anc, ref = _case(N, dev)
    got = tr.logpdf_device(th[:M].contiguous(), hint=anc[:M].contiguous()).cpu().numpy()
    err = np.abs(np.exp(got - ref[:M]) - 1.0).max()
    got2 = tr.logpdf_device(th[:M].contiguous()).cpu().numpy()
    err2 = np.abs(np.exp(got2 - ref[:M]) - 1.0).max()
    print(f"N={N} M={M}: max rel err hinted {err:.3e}, unhinted {err2:.3e}")
    np.testing.assert_allclose(np.exp(got - ref[:M]), 1.0, rtol=1e-6, atol=0)
    np.testing.assert_allclose(np.exp(got2 - ref[:M]), 1.0, rtol=1e-6, atol=0)


@pytest.mark.parametrize("hinted", [True, False])
def test_x3_position_independence(dev, hinted):
    """A candidate's bits depend neither on how many candidates the call has
    nor on its slot: all 769, the first 100 alone, and the set reversed."""
    tr, th, anc, ref = _case(1280, dev)

    def run(idx):
        x = th[idx].contiguous()
        h = anc[idx].contiguous() if hinted else None
        return tr.logpdf_device(x, hint=h).cpu().numpy().view(np.int64)

    allc = torch.arange(M_MAX, device=th.device)
    full = run(allc)
    first = run(allc[:100])
    rev = run(torch.flip(allc, dims=[0]))
    np.testing.assert_array_equal(first, full[:100])
    np.testing.assert_array_equal(rev[::-1], full)
