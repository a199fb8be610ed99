"""Generate tests/golden/measure_list.npz by importing the pyABC 0.10.5 reference.

Runs in the build container only, with the reference checkout and this
directory on PYTHONPATH (like make_golden_aggregated.py); never on the GPU
box, and nothing here is imported by the product.

    PYTHONDONTWRITEBYTECODE=1 OMP_NUM_THREADS=1 \
      PYTHONPATH=<pyabc 0.10.5 checkout>:tests/golden \
      python tests/golden/make_golden_measure_list.py

Data only.  Samples are stored as float32 (every value exact in float64, half
the bytes); the reference saw them as float64.

    A__sample [2000, 10]   column scales over two decades, non-zero means
    B__sample [2000, 10]   rotated: cond_2 of the centred Gram matrix ~ 1e4
    C__sample [40, 3]
    {A,B,C}__x0 [S], {A,B,C}__rows [200, S]   observation and test rows
For every sample T and class in (zscore, pca, minmax, percentile):
    T_minmax__norm, T_percentile__norm [S]    normalization in key order
    T_pca__W [S, S]                           the whitening matrix
    T_{class}__d [200]                        reference distances of the rows
The measures_to_use case (sample A, SUBSET, not in x_0 order):
    SUBSET                                    the key indices
    A_sub_minmax__norm, A_sub_percentile__norm [3] (SUBSET order),
    A_sub_pca__W [3, 3], A_sub_{class}__d [200]
ZScore with a zero observation (sample C's rows, some entries exactly 0):
    Z__x0 [3], Z__rows [200, 3], Z_zscore__d [200] (inf where only x_0 is 0)
"""
import os

import numpy as np

import stub_env  # noqa: F401  (must precede pyabc)
from pyabc.distance import (MinMaxDistance, PCADistance, PercentileDistance,
                            ZScoreDistance)

HERE = os.path.dirname(os.path.abspath(__file__))
CLASSES = {"zscore": ZScoreDistance, "pca": PCADistance, "minmax": MinMaxDistance,
           "percentile": PercentileDistance}
SUBSET = [7, 2, 5]


def keys(S):
    return [f"y{k}" for k in range(S)]


def as_dicts(data):
    ks = keys(data.shape[1])
    return [dict(zip(ks, row)) for row in data]


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def run(out, tag, sample, x0, rows, measures="all"):
    ks = keys(sample.shape[1])
    stats = as_dicts(sample)
    x0d = dict(zip(ks, x0))
    for name, cls in CLASSES.items():
        dist = cls(measures_to_use=measures)
        dist.initialize(0, lambda: stats, x0d)
        use = list(dist.measures_to_use)
        if name in ("minmax", "percentile"):
            out[f"{tag}_{name}__norm"] = np.array([dist.normalization[k] for k in use])
        if name == "pca":
            out[f"{tag}_pca__W"] = dist._whitening_transformation_matrix
        out[f"{tag}_{name}__d"] = np.array([dist(r, x0d) for r in as_dicts(rows)],
                                           dtype=np.float64)


def main():
    rng = np.random.default_rng(20261020)
    out = {}
    S = 10
    scales = np.logspace(-1, 1, S)
    means = rng.uniform(2.0, 5.0, size=S) * scales
    A = f32(rng.normal(size=(2000, S)) * scales + means)
    # B: singular values over one decade squared -> cond_2(G) ~ 1e4
    q, _ = np.linalg.qr(rng.normal(size=(S, S)))
    B = f32((rng.normal(size=(2000, S)) * np.logspace(0, -2, S)) @ q.T + means)
    C = f32(rng.normal(size=(40, 3)) * [0.5, 2.0, 1.0] + [1.0, -3.0, 2.0])
    for tag, sample in (("A", A), ("B", B), ("C", C)):
        s = sample.shape[1]
        x0 = sample.mean(axis=0) + 0.3 * sample.std(axis=0) * rng.normal(size=s)
        rows = sample.mean(axis=0) + 1.5 * sample.std(axis=0) * rng.normal(size=(200, s))
        if tag == "B":
            rows = sample[rng.integers(0, 2000, size=200)] + \
                0.1 * (rng.normal(size=(200, s)) * np.logspace(0, -2, s)) @ q.T
        out[f"{tag}__sample"] = sample.astype(np.float32)
        out[f"{tag}__x0"] = x0
        out[f"{tag}__rows"] = rows
        run(out, tag, sample, x0, rows)
    out["SUBSET"] = np.array(SUBSET)
    run(out, "A_sub", A, out["A__x0"], out["A__rows"],
        measures=[f"y{k}" for k in SUBSET])
    # ZScore with a zero observation: key 1 observed as 0; rows 0..49 also 0 there
    zx0 = out["C__x0"].copy()
    zx0[1] = 0.0
    zrows = out["C__rows"].copy()
    zrows[:50, 1] = 0.0
    out["Z__x0"], out["Z__rows"] = zx0, zrows
    z = ZScoreDistance()
    x0d = dict(zip(keys(3), zx0))
    z.initialize(0, lambda: as_dicts(C), x0d)
    with np.errstate(all="ignore"):
        out["Z_zscore__d"] = np.array([z(r, x0d) for r in as_dicts(zrows)], dtype=np.float64)
    path = os.path.join(HERE, "measure_list.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    G = (A - A.mean(0)).T @ (A - A.mean(0))
    GB = (B - B.mean(0)).T @ (B - B.mean(0))
    print("cond A", np.linalg.cond(G), "cond B", np.linalg.cond(GB))


if __name__ == "__main__":
    main()
