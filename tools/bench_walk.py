"""DiscreteRandomWalkTransition on the device: the density kernel and one
generation of the batched sampler over an integer parameter.

    python tools/bench_walk.py [--reps 5] [--host-n 10000] [--pop 100000]
        [--skip-large] [--out FILE]

  density     abc_walk_logpmf (with its chunk-combining kernel) at
              (N = M = 1e5, d = 5, n_steps = 2) and (N = M = 1e6, d = 2,
              n_steps = 2): a clustered population (Poisson(20) per
              coordinate, Gamma weights), the candidates its own proposals.
              HIP-event milliseconds after one warm-up, median (min, max) of
              --reps calls; pairs/s = M N / median.  "near" is the fraction
              of pairs within n_steps in every coordinate (counted on a
              sample of candidates), the ones whose law entries are gathered.
  host        the numpy form of the same class (the per-candidate loop's
              density) on the first --host-n rows of the d = 5 arrays, wall
              clock, and the largest difference of the two forms there.
  generation  y = k + 0.5 noise, prior poisson(3), n_steps = 2, population
              --pop: wall seconds (device synchronised) of each generation's
              sampling call, weights included, and candidates per second.

One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def population(N, d, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.poisson(20.0, size=(N, d)).astype(np.float64)
    w = rng.gamma(1.0, size=N)
    return X, w / w.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=10000)
    ap.add_argument("--pop", type=int, default=100000)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pandas as pd
    import torch
    import pyabc_amd as pa
    from pyabc_amd import gpu
    gpu.require_device()
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    shapes = [(10 ** 5, 5)] + ([] if a.skip_large else [(10 ** 6, 2)])
    for N, d in shapes:
        X, w = population(N, d)
        cols = [f"p{k}" for k in range(d)]
        tr = pa.DiscreteRandomWalkTransition(n_steps=2)
        tr.fit_device(gpu.as_dev(X), gpu.as_dev(w), cols)
        x = tr.propose_device(N, seed=3, idx0=0)[0]
        out = torch.empty(N, dtype=torch.float64, device=x.device)
        tr.logpdf_device(x, out=out)                              # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.logpdf_device(x, out=out)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        xs = x[:64].cpu().numpy()
        near = float((np.abs(xs[:, None, :] - X[None, :, :]) <= 2).all(axis=2).mean())
        med = float(np.median(ms))
        emit({"what": "density", "N": N, "M": N, "d": d, "n_steps": 2, "reps": a.reps,
              "ms": {"median": med, "min": float(min(ms)), "max": float(max(ms))},
              "pairs_per_s": N * N / (med * 1e-3), "near_fraction": near,
              "chunk": gpu.walk_logpmf_chunk(N, N, d),
              "finite": int(torch.isfinite(out).sum().item())})
        if d == 5 and a.host_n:
            n = min(a.host_n, N)
            host = pa.DiscreteRandomWalkTransition(n_steps=2)
            wn = w[:n] / w[:n].sum()
            host.fit(pd.DataFrame(X[:n], columns=cols), wn.copy())
            xh = pd.DataFrame(x[:n].cpu().numpy(), columns=cols)
            t0 = time.perf_counter()
            ph = host.pdf(xh)
            sec = time.perf_counter() - t0
            dev = pa.DiscreteRandomWalkTransition(n_steps=2)
            dev.fit_device(gpu.as_dev(X[:n]), gpu.as_dev(wn), cols)
            pd_ = torch.exp(dev.logpdf_device(x[:n].contiguous())).cpu().numpy()
            rel = np.abs(pd_ - ph)[ph > 0] / ph[ph > 0]
            emit({"what": "host", "N": n, "M": n, "d": d, "n_steps": 2, "seconds": sec,
                  "pairs_per_s": n * n / sec,
                  "max_rel_diff_device": float(rel.max()) if len(rel) else 0.0,
                  "zeros_equal": bool(np.array_equal(pd_ == 0, ph == 0))})

    # one generation of the sampler test's model
    from test_gpu_walk import SIGMA, _noise

    def sim(theta, seed, gen, idx0):
        return theta + SIGMA * _noise(theta, seed, gen, idx0)

    sampler = pa.BatchedGPUSampler(seed=11, allow_per_candidate=False)
    abc = pa.ABCSMC(pa.VectorizedModel(sim, ["y"]), pa.Distribution(k=pa.RV("poisson", 3)),
                    pa.PNormDistance(p=2), population_size=a.pop, sampler=sampler,
                    transitions=pa.DiscreteRandomWalkTransition(n_steps=2),
                    eps=pa.MedianEpsilon())
    abc.new("sqlite://", {"y": 4.0})
    inner, calls = sampler.sample_until_n_accepted, []

    def timed(*args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = inner(*args, **kw)
        torch.cuda.synchronize()
        calls.append((time.perf_counter() - t0, dict(sampler.last_stats)))
        return res
    sampler.sample_until_n_accepted = timed
    abc.run(max_nr_populations=4)
    for g, (sec, st) in enumerate(calls):
        emit({"what": "generation", "call": g, "population": a.pop, "seconds": sec,
              "evaluations": int(st.get("evaluations", 0)),
              "candidates_per_s": st.get("evaluations", 0) / sec,
              "per_candidate": bool(st.get("per_candidate", False))})
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
