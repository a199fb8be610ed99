"""Generate tests/golden/randomwalk.npz by importing the pyABC 0.10.5 reference.

Runs in the build container only, with the reference checkout and this
directory on PYTHONPATH (like make_golden_models.py); never on the GPU box,
and nothing here is imported by the product.

    PYTHONDONTWRITEBYTECODE=1 OMP_NUM_THREADS=1 \
      PYTHONPATH=<pyabc 0.10.5 checkout>:tests/golden \
      python tests/golden/make_golden_randomwalk.py

DiscreteRandomWalkTransition.pdf (pyabc/transition/randomwalk.py:55-81):

    X [40, 2], w [40]     a weighted integer population (columns "a", "b")
    x [30, 2]             candidates: some near particles, some far away
    settings [3, 4]       (n_steps, p_l, p_r, p_c) per case
    pdf [3, 30]           the reference's pdf of every candidate per setting
"""
import os

import numpy as np
import pandas as pd

import stub_env  # noqa: F401  (must precede pyabc)
from pyabc.transition import DiscreteRandomWalkTransition

HERE = os.path.dirname(os.path.abspath(__file__))
SETTINGS = [(1, 1. / 3, 1. / 3, 1. / 3), (3, .25, .35, .4), (4, .5, .5, 0.)]


def gen():
    rng = np.random.default_rng(20240611)
    X = rng.integers(-3, 9, size=(40, 2)).astype(np.float64)
    w = rng.random(40)
    w /= w.sum()
    x = X[rng.integers(0, 40, size=30)] + rng.integers(-3, 4, size=(30, 2))
    x[-4:] += 40.0                      # further than any walk reaches
    Xdf = pd.DataFrame(X, columns=["a", "b"])
    xdf = pd.DataFrame(x, columns=["a", "b"])
    out = np.empty((len(SETTINGS), len(x)))
    for c, (n, p_l, p_r, p_c) in enumerate(SETTINGS):
        tr = DiscreteRandomWalkTransition(n_steps=n, p_l=p_l, p_r=p_r, p_c=p_c)
        tr.fit(Xdf, w.copy())
        out[c] = [tr.pdf(xdf.iloc[i]) for i in range(len(x))]
    return dict(X=X, w=w, x=x, settings=np.array(SETTINGS), pdf=out)


if __name__ == "__main__":
    np.savez(os.path.join(HERE, "randomwalk.npz"), **gen())
