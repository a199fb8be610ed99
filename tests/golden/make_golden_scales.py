"""Generate tests/golden/scales.npz by importing the pyABC 0.10.5 reference.

Runs in the build container only, with the reference checkout and this
directory on PYTHONPATH (like make_golden.py); never on the GPU box, and
nothing here is imported by the product.

    PYTHONDONTWRITEBYTECODE=1 OMP_NUM_THREADS=1 \
      PYTHONPATH=<pyabc 0.10.5 checkout>:tests/golden \
      python tests/golden/make_golden_scales.py

For R in {100, 101} recorded samples of S = 12 summary statistics (the
adaptive.npz construction: a constant column, a rounded column with ties) and
a non-trivial observation x0, the ten sum-stat scale functions of
pyabc/distance/scale.py:38-135 per key, and the weights
AdaptivePNormDistance.initialize makes of them with max_weight_ratio None
and 5.

    R{R}__data [R, S], R{R}__x0 [S]
    R{R}_{function}__scales [S]
    R{R}_{function}_r{ratio}__w [S]
"""
import os

import numpy as np

import stub_env  # noqa: F401  (must precede pyabc)
from pyabc.distance import AdaptivePNormDistance
from pyabc.distance import scale as ref_scale

HERE = os.path.dirname(os.path.abspath(__file__))

FUNCTIONS = ["median_absolute_deviation", "mean_absolute_deviation",
             "standard_deviation", "bias", "root_mean_square_deviation",
             "median_absolute_deviation_to_observation",
             "mean_absolute_deviation_to_observation",
             "combined_median_absolute_deviation",
             "combined_mean_absolute_deviation",
             "standard_deviation_to_observation"]
S = 12
CONST = 4.2


def gen_scales():
    rng = np.random.default_rng(11)
    res = {}
    for R in (101, 100):
        keys = [f"y{k}" for k in range(S)]
        mag = 10.0 ** rng.uniform(-2, 2, size=S)
        data = rng.normal(size=(R, S)) * mag
        data[:, 3] = CONST                  # zero-scale key -> weight 0
        data[:, 5] = np.round(data[:, 5])   # ties for the medians
        x0v = rng.normal(size=S) * mag
        x0v[0] = data[7, 0]                 # equal to one data value
        x0v[5] = data[0, 5]                 # equal to a tied data value
        x0v[3] = CONST                      # the constant column's value
        x0v[8] = data[:, 8].mean() + 1e3 * data[:, 8].std()   # 1e3 sigma away
        x0v[10] = np.median(data[:, 10])    # the column's own median
        x0 = {k: float(v) for k, v in zip(keys, x0v)}
        ss = [{k: float(v) for k, v in zip(keys, row)} for row in data]
        res[f"R{R}__data"] = data
        res[f"R{R}__x0"] = np.array([x0[k] for k in keys])
        for name in FUNCTIONS:
            sf = getattr(ref_scale, name)
            scales = np.array([sf(data=[s[k] for s in ss], x_0=x0[k])
                               for k in keys], dtype=np.float64)
            # no scale near np.isclose(scale, 0)'s threshold: the weights do
            # not hinge on a last-bit difference
            assert np.all((scales == 0) | (scales > 1e-6)), (name, scales)
            res[f"R{R}_{name}__scales"] = scales
            for ratio in (None, 5.0):
                dist = AdaptivePNormDistance(scale_function=sf,
                                             max_weight_ratio=ratio)
                dist.initialize(0, lambda: ss, x0)
                res[f"R{R}_{name}_r{ratio}__w"] = np.array(
                    [dist.weights[0][k] for k in keys], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "scales.npz"), **res)
    print("scales", len(res), "arrays")


if __name__ == "__main__":
    gen_scales()
