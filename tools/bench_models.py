"""One multi-model candidate round against the single-model staged round.

    python tools/bench_models.py [--B 2000000] [--N 50000] [--reps 7] [--out FILE]

A round is what BatchedGPUSampler runs per iteration of its staged loops,
without the kept-row gather: proposal -> simulator -> one-pass accept tail.

  models   M = 2 (d = 10 and 6, N particles each, q~ = (1/2, 1/2), norm
           priors), S = 10: abc_models_propose ->
           abc_models_simulate_linear_gaussian -> abc_pnorm_accept
  single   the unchanged single-model staged round at the same B (d = 10, the
           first model alone): abc_candidates_propose ->
           abc_simulate_linear_gaussian -> abc_pnorm_accept

Times are HIP-event milliseconds around a round, after a warm-up of both
variants, the two alternated within each repetition; the median and the
spread (min, max) are reported as candidates per second.  One JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def population(rng, N, d):
    X = 0.3 + rng.standard_normal((N, d))
    w = rng.gamma(2.0, size=N)
    A = rng.standard_normal((d, d))
    L = np.linalg.cholesky(A @ A.T / d + np.eye(d)) * 0.3
    return X, w / w.sum(), L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=2_000_000)
    ap.add_argument("--N", type=int, default=50_000)
    ap.add_argument("--S", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pyabc_amd import gpu
    dev = gpu.require_device()
    rng = np.random.default_rng(3)
    dims, S, B = (10, 6), a.S, a.B
    descs, tabs = [], []
    for d in dims:
        X, w, L = population(rng, a.N, d)
        cdf = gpu.inclusive_scan(gpu.as_dev(w))
        descs.append(dict(
            d=d, X=gpu.as_dev(X), cdf=cdf, guide=gpu.cdf_guide(cdf), L=gpu.as_dev(L),
            prior_kind=torch.zeros(d, dtype=torch.int32, device=dev),
            prior_params=gpu.as_dev(np.tile([0.0, 10.0, 0, 0], d))))
        tabs.append((np.arange(S) % d, np.ones(S), np.full(S, 0.5)))
    src = gpu.as_dev(np.stack([t[0] for t in tabs]), dtype=torch.int32)
    av = gpu.as_dev(np.stack([t[1] for t in tabs]))
    sg = gpu.as_dev(np.stack([t[2] for t in tabs]))
    x0 = gpu.as_dev(np.full(S, 0.3))
    wf = gpu.as_dev(np.ones(S))
    eps, cap = 1.5, B
    ms = gpu.ModelSet(descs, [0.5, 1.0], 11, 1, 1000)
    one = descs[0]
    fr = gpu.CandidateRound(dims[0], S, one["prior_kind"], one["prior_params"],
                            src[0].contiguous(), av[0].contiguous(), sg[0].contiguous(), x0,
                            wf, 2.0, 11, 1, 1000, X=one["X"], cdf=one["cdf"],
                            guide=one["guide"], L=one["L"])

    def models():
        model, theta, anc, att = ms.propose(0, B)
        x = gpu.models_simulate_linear_gaussian(theta, model, src, av, sg, 11, 1, 0)
        return gpu.pnorm_accept(x, x0, wf, 2.0, eps, cap, att=att, max_attempts=1000)[1]

    def single():
        theta, _, anc, att = fr.propose(0, B, with_lp=False)
        x = gpu.simulate_linear_gaussian(theta, src[0], av[0], sg[0], 11, 1, 0)
        return gpu.pnorm_accept(x, x0, wf, 2.0, eps, cap, att=att, max_attempts=1000)[1]

    variants = {"models": models, "single": single}
    accepted = {k: int(f().item()) for k, f in variants.items()}      # warm-up
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, f in variants.items():                                   # alternated
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1))
    line = {"B": B, "N": a.N, "S": S, "dims": list(dims), "reps": a.reps,
            "accepted": accepted}
    for k, v in t.items():
        line[f"{k}_ms"] = {"median": float(np.median(v)), "min": float(min(v)),
                           "max": float(max(v))}
        line[f"{k}_candidates_per_s"] = {
            "median": B / (1e-3 * float(np.median(v))),
            "min": B / (1e-3 * float(max(v))), "max": B / (1e-3 * float(min(v)))}
    line["models_over_single_time"] = line["models_ms"]["median"] / line["single_ms"]["median"]
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
