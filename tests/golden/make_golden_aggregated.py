"""Generate tests/golden/aggregated.npz by importing the pyABC 0.10.5 reference.

Runs in the build container only, with the reference checkout and this
directory on PYTHONPATH (like make_golden_scales.py); never on the GPU box,
and nothing here is imported by the product.

    PYTHONDONTWRITEBYTECODE=1 OMP_NUM_THREADS=1 \
      PYTHONPATH=<pyabc 0.10.5 checkout>:tests/golden \
      python tests/golden/make_golden_aggregated.py

For R in {100, 101} recorded samples of S = 12 summary statistics
(make_golden_scales.py's construction: a constant column, a rounded column
with ties) and three children -- PNormDistance(p=1) on keys 0..3,
PNormDistance(p=2) on keys 4..11, AdaptivePNormDistance(p=inf) on all keys --
the per-row terms, AggregatedDistance.__call__ for list and dict-by-t weights
and factors (pyabc/distance/distance.py:445-461) and the weights
AdaptiveAggregatedDistance makes in initialize and after one update
(distance.py:556-625) with span, mean and median (scale.py:138-151).

    R{R}__data, R{R}__data2 [R, S], R{R}__x0 [S]
    R{R}__child2_w [S]          the adaptive child's weights after initialize
    R{R}__terms [R, 3]          children's distances of the rows of data
    LIST_W, LIST_F [3]; R{R}_list__d [R]
    DICT_W_t0, DICT_W_t2, DICT_F_t0 [3]; R{R}_dict_t{0,2,5}__d [R]
    R{R}_{function}__w0, __w1 [3]; R{R}_{function}__child2_w1 [S]
"""
import os

import numpy as np

import stub_env  # noqa: F401  (must precede pyabc)
from pyabc.distance import (AdaptiveAggregatedDistance, AdaptivePNormDistance,
                            AggregatedDistance, PNormDistance)
from pyabc.distance import scale as ref_scale

HERE = os.path.dirname(os.path.abspath(__file__))

S = 12
CONST = 4.2
KEYS = [f"y{k}" for k in range(S)]
LIST_W = [1.0, 0.5, 2.0]
LIST_F = [2.0, 1.0, 0.25]
DICT_W = {0: [1.0, 0.5, 2.0], 2: [0.3, 1.7, 0.9]}
DICT_F = {0: [1.5, 1.0, 0.5]}


def children():
    return [PNormDistance(p=1, weights={k: 1.0 for k in KEYS[:4]}),
            PNormDistance(p=2, weights={k: 1.0 for k in KEYS[4:]}),
            AdaptivePNormDistance(p=np.inf)]


def sample(rng, R, mag):
    data = rng.normal(size=(R, S)) * mag
    data[:, 3] = CONST                  # zero-scale key -> weight 0
    data[:, 5] = np.round(data[:, 5])   # ties for the medians
    return data


def as_dicts(data):
    return [{k: float(v) for k, v in zip(KEYS, row)} for row in data]


def check_scales(name, fn, cols):
    """No comparison may hinge on cancellation in a span or on np.isclose's
    threshold in the weights."""
    for col in cols:
        assert max(col) - min(col) > 1e-3 * max(col), (name, "span margin")
        scale = fn(col)
        assert not (0 < scale < 1e-6), (name, scale)


def gen():
    rng = np.random.default_rng(23)
    res = {"LIST_W": np.array(LIST_W), "LIST_F": np.array(LIST_F),
           "DICT_W_t0": np.array(DICT_W[0]), "DICT_W_t2": np.array(DICT_W[2]),
           "DICT_F_t0": np.array(DICT_F[0])}
    for R in (101, 100):
        mag = 10.0 ** rng.uniform(-2, 2, size=S)
        data, data2 = sample(rng, R, mag), sample(rng, R, 1.5 * mag)
        x0v = rng.normal(size=S) * mag
        x0v[3] = CONST
        x0 = {k: float(v) for k, v in zip(KEYS, x0v)}
        ss, ss2 = as_dicts(data), as_dicts(data2)
        res[f"R{R}__data"], res[f"R{R}__data2"] = data, data2
        res[f"R{R}__x0"] = x0v

        agg = AggregatedDistance(children(), weights=list(LIST_W), factors=list(LIST_F))
        agg.initialize(0, lambda: ss, x0)
        res[f"R{R}__child2_w"] = np.array([agg.distances[2].weights[0][k] for k in KEYS])
        res[f"R{R}__terms"] = np.array([[d(s, x0, 0) for d in agg.distances] for s in ss])
        res[f"R{R}_list__d"] = np.array([agg(s, x0, 0) for s in ss])

        agg = AggregatedDistance(children(),
                                 weights={t: np.array(w) for t, w in DICT_W.items()},
                                 factors={t: np.array(f) for t, f in DICT_F.items()})
        agg.initialize(0, lambda: ss, x0)
        for t in (0, 2, 5):             # 5: falls back to the latest entry
            res[f"R{R}_dict_t{t}__d"] = np.array([agg(s, x0, t) for s in ss])

        for name in ("span", "mean", "median"):
            fn = getattr(ref_scale, name)
            ada = AdaptiveAggregatedDistance(children(), scale_function=fn)
            ada.initialize(0, lambda: ss, x0)
            check_scales(name, fn, [[d(s, x0) for s in ss] for d in ada.distances])
            res[f"R{R}_{name}__w0"] = np.array(ada.weights[0], dtype=np.float64)
            assert ada.update(1, lambda: ss2)
            check_scales(name, fn, [[d(s, x0) for s in ss2] for d in ada.distances])
            res[f"R{R}_{name}__w1"] = np.array(ada.weights[1], dtype=np.float64)
            res[f"R{R}_{name}__child2_w1"] = np.array(
                [ada.distances[2].weights[1][k] for k in KEYS])
    np.savez_compressed(os.path.join(HERE, "aggregated.npz"), **res)
    print("aggregated", len(res), "arrays")


if __name__ == "__main__":
    gen()
