"""GridSearchCV: the fused scaled-KDE route against one fit + density per
grid point and fold, and against the host restatement.

    python tools/bench_gridsearch.py [--N 10000,100000] [--d 10] [--cv 5]
        [--reps 5] [--host-max 10000] [--out FILE]

At each N (default grid of 5 scalings, correlated Gaussian population, Gamma
weights) it times, test scores only and without the refit:

  device   GridSearchCV.fit_device: per fold one abc_weighted_moments +
           abc_mvn_fit and one abc_mvn_logpdf_scaled call for all scalings
  generic  the same search on the existing kernels: per fold and grid point
           MultivariateNormalTransition.fit_device + logpdf_device + the
           weighted sum, at precision "x3" (the default) and "f64" (the
           arithmetic the fused kernel uses)
  train    the device route with return_train_score=True (4x the pairs)
  host     tests/gridsearch_ref.py (numpy float64), N <= --host-max only

Times are HIP-event milliseconds around the whole search, after one warm-up
of every variant, the variants alternated within each repetition; the median
and the spread (min, max) are reported.  One JSON line per N.
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
    A = rng.normal(size=(d, d)) + 2 * np.eye(d)
    X = rng.normal(size=(N, d)) @ A.T
    w = rng.gamma(1.0, size=N)
    return X, w / w.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", default="10000,100000")
    ap.add_argument("--d", type=int, default=10)
    ap.add_argument("--cv", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=10000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pyabc_amd import gpu
    from pyabc_amd.transition import GridSearchCV, MultivariateNormalTransition
    from pyabc_amd.transition.model_selection import kfold_bounds
    import gridsearch_ref as ref
    gpu.require_device()
    scalings = np.linspace(0.05, 1.0, 5)
    cols = [f"p{k}" for k in range(a.d)]
    lines = []
    for N in (int(v) for v in a.N.split(",")):
        X, w = population(N, a.d)
        Xd, wd = gpu.as_dev(X), gpu.as_dev(w)
        folds = kfold_bounds(N, a.cv)

        def device(train=False):
            gs = GridSearchCV(cv=a.cv, refit=False, return_train_score=train)
            gs.fit_device(Xd, wd, cols)
            assert gs.route_ == "device"
            return np.stack([gs.cv_results_[f"split{f}_test_score"]
                             for f in range(a.cv)], axis=1)

        def generic(prec):
            sc = []
            for lo, hi in folds:
                Xtr = torch.cat((Xd[:lo], Xd[hi:])).contiguous()
                wtr = torch.cat((wd[:lo], wd[hi:]))
                wtr = (wtr / wtr.sum()).contiguous()
                for s in scalings:
                    est = MultivariateNormalTransition(scaling=float(s), precision=prec)
                    est.fit_device(Xtr, wtr, cols)
                    sc.append((est.logpdf_device(Xd[lo:hi]) * wd[lo:hi]).sum())
            return torch.stack(sc).cpu().numpy().reshape(a.cv, -1).T

        variants = {"device": device, "generic_x3": lambda: generic("x3"),
                    "generic_f64": lambda: generic("f64"),
                    "device_train": lambda: device(True)}
        scores = {k: f() for k, f in variants.items()}          # warm-up
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, f in variants.items():                       # alternated
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        line = {"N": N, "d": a.d, "cv": a.cv, "G": len(scalings), "reps": a.reps,
                "test_pairs": int(sum((hi - lo) * (N - (hi - lo)) for lo, hi in folds))
                * len(scalings)}
        for k, v in ms.items():
            line[f"{k}_ms"] = {"median": float(np.median(v)), "min": float(min(v)),
                               "max": float(max(v))}
        line["device_over_generic_x3"] = line["device_ms"]["median"] / line["generic_x3_ms"]["median"]
        line["device_over_generic_f64"] = line["device_ms"]["median"] / line["generic_f64_ms"]["median"]
        for k in ("generic_x3", "generic_f64", "device_train"):
            line[f"max_score_diff_{k}"] = float(np.abs(scores[k] - scores["device"]).max())
        if N <= a.host_max:
            t0 = time.perf_counter()
            host, _ = ref.grid_search(X, w, scalings, a.cv)
            line["host_numpy_ms"] = 1e3 * (time.perf_counter() - t0)
            line["max_score_diff_host"] = float(np.abs(host - scores["device"]).max())
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
