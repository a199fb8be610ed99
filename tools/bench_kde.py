"""The KDE matrix: one abc_kde_panels call for all panels against one fit +
density per panel on the existing kernels, and against the host form.

    python tools/bench_kde.py [--shapes 10:1000000,5:100000] [--num 50]
        [--reps 5] [--host-N 10000] [--out FILE]

At each shape d:N (correlated Gaussian population, Gamma weights, the
d (d + 1) / 2 panels of plot_kde_matrix on num x num grids) it times

  one_call   visualization.kde_matrix: one abc_weighted_moments, the host
             plan, one abc_kde_panels, the densities read back
  kernel     the abc_kde_panels call alone (plan and descriptors ready)
  per_panel  per panel a column gather, MultivariateNormalTransition
             .fit_device and .logpdf_device on the panel's grid, at precision
             "x3" (the default) and "f64", the densities read back

and, once, the host form of the reference (a Python loop over the grid points
of scipy's frozen normal against every particle) for one 2-D panel at
--host-N particles.  Times are HIP-event milliseconds after one warm-up of
every variant, the variants alternated within each repetition; median and
spread (min, max).  terms = grid points x particles.  One JSON line per shape.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def population(N, d, seed=5):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(d, d)) + 2 * np.eye(d)
    X = rng.normal(size=(N, d)) @ A.T
    w = rng.gamma(1.0, size=N)
    return X, w / w.sum()


def host_panel(X, w, num):
    """kde_2d as the reference evaluates it, on the host."""
    import scipy.stats as st
    N = len(X)
    ess = 1 / np.sum(w ** 2)
    cov = np.cov(X, aweights=w, rowvar=False) * (4 / ess / 4) ** (2 / 6)
    normal = st.multivariate_normal(cov=cov, allow_singular=True)
    gx, gy = np.meshgrid(np.linspace(X[:, 0].min(), X[:, 0].max(), num),
                         np.linspace(X[:, 1].min(), X[:, 1].max(), num))
    pts = np.stack([gx.ravel(), gy.ravel()], axis=1)
    t0 = time.perf_counter()
    dens = np.array([(normal.pdf(p - X) * w).sum() for p in pts])
    return 1e3 * (time.perf_counter() - t0), dens.reshape(gx.shape), N * pts.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10:1000000,5:100000")
    ap.add_argument("--num", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-N", type=int, default=10000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pandas as pd
    import torch
    from pyabc_amd import gpu
    from pyabc_amd import visualization as vis
    from pyabc_amd.population import ColumnarParticles
    from pyabc_amd.transition import MultivariateNormalTransition
    gpu.require_device()
    lines = []
    for shape in a.shapes.split(","):
        d, N = (int(v) for v in shape.split(":"))
        X, w = population(N, d)
        names = [f"p{k}" for k in range(d)]
        Xd, wd = gpu.as_dev(X), gpu.as_dev(w)
        cols = ColumnarParticles.__new__(ColumnarParticles)
        cols.theta, cols.weights, cols.param_names = Xd, wd, names

        def one_call():
            return vis.kde_matrix(cols, None, None, a.num, a.num)

        first = one_call()
        assert set(first.panel_routes_.values()) == {"kernel"}
        sw, sw2, mean, cov_b = gpu.weighted_moments(Xd, wd)
        plan = vis.plan_panels(names, cov_b * sw / (sw - sw2 / sw), 1 / sw2, X.min(axis=0),
                               X.max(axis=0), None, a.num, a.num, mean=mean, n_particles=N)
        desc = plan.descriptors()

        def kernel():
            return gpu.kde_panels(Xd, wd, desc, plan.coords)

        def per_panel(prec):
            out = {}
            for q in plan.panels:
                sub = Xd[:, q["cols"]].contiguous()
                est = MultivariateNormalTransition(precision=prec)
                est.fit_device(sub, wd, list(q["key"]))
                if len(q["key"]) == 1:
                    pts = q["axes"][0][:, None]
                else:
                    gx, gy = np.meshgrid(*q["axes"])
                    pts = np.stack([gx.ravel(), gy.ravel()], axis=1)
                out[q["key"]] = torch.exp(est.logpdf_device(gpu.as_dev(pts))).cpu().numpy()
            return out

        variants = {"one_call": one_call, "kernel": kernel,
                    "per_panel_x3": lambda: per_panel("x3"),
                    "per_panel_f64": lambda: per_panel("f64")}
        res = {k: f() for k, f in variants.items()}              # warm-up
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, f in variants.items():                        # alternated
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        G = plan.n_points
        line = {"d": d, "N": N, "num": a.num, "panels": len(plan.panels), "grid_points": G,
                "terms": G * N, "reps": a.reps,
                "workspace_bytes": gpu.kde_panels_bytes(N, d, len(plan.panels), G)}
        for k, v in ms.items():
            line[f"{k}_ms"] = {"median": float(np.median(v)), "min": float(min(v)),
                               "max": float(max(v))}
            line[f"{k}_terms_per_s"] = G * N / (1e-3 * float(np.median(v)))
        for k in ("x3", "f64"):
            line[f"one_call_over_per_panel_{k}"] = (line["one_call_ms"]["median"]
                                                    / line[f"per_panel_{k}_ms"]["median"])
            worst = 0.0
            for key, val in res[f"per_panel_{k}"].items():
                mine = first[key][-1].ravel()
                big = mine > 1e-200
                worst = max(worst, float(np.max(np.abs(val[big] / mine[big] - 1))))
            line[f"max_rel_diff_per_panel_{k}"] = worst
        print(json.dumps(line), flush=True)
        lines.append(line)
    Xh, wh = population(a.host_N, 2)
    host_ms, dens, terms = host_panel(Xh, wh, a.num)
    mine = vis.kde_2d(pd.DataFrame(Xh, columns=["p0", "p1"]), wh.copy(), "p0", "p1",
                      numx=a.num, numy=a.num)[2]
    big = dens > 1e-200
    line = {"host_form": "one 2-D panel, Python loop over grid points", "N": a.host_N,
            "num": a.num, "terms": terms, "host_ms": host_ms,
            "host_terms_per_s": terms / (1e-3 * host_ms),
            "max_rel_diff_device": float(np.max(np.abs(mine[big] / dens[big] - 1)))}
    print(json.dumps(line), flush=True)
    lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
