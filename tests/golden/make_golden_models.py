"""Generate tests/golden/models.npz by importing the pyABC 0.10.5 reference.

Runs in the build container only, with the reference checkout and this
directory on PYTHONPATH (like make_golden_aggregated.py); never on the GPU
box, and nothing here is imported by the product.

    PYTHONDONTWRITEBYTECODE=1 OMP_NUM_THREADS=1 \
      PYTHONPATH=<pyabc 0.10.5 checkout>:tests/golden \
      python tests/golden/make_golden_models.py

The model steps of a run with several models:

    pmf_M{M}_stay{tag} [M + 1, M]   ModelPerturbationKernel(M, stay).pmf(n, m),
                                    n = 0 .. M (n == M: mass 0), m = 0 .. M - 1
                                    (random_variables.py:513-538); tag in
                                    none, 0.7, 1.0
    P_PREV [3]                      previous model probabilities (0.2, 0, 0.8)
    factor_stay{tag} [3]            ABCSMC._create_transition_pdf's model
                                    factor for target m = 0, 1, 2 (smc.py:
                                    739-746, particle factor 1)
    NORM_m [12], NORM_w [12]        hand-made particles over 3 models
    NORM_w_out [12]                 their weights after
                                    Population._normalize_weights
                                    (population.py:123-145)
    NORM_p [3]                      get_model_probabilities
    NORM_wd [12]                    get_weighted_distances().w
"""
import os

import numpy as np
import pandas as pd

import stub_env  # noqa: F401  (must precede pyabc)
from pyabc.parameters import Parameter
from pyabc.population import Particle, Population
from pyabc.random_variables import ModelPerturbationKernel
from pyabc.smc import ABCSMC

HERE = os.path.dirname(os.path.abspath(__file__))
STAYS = {"none": None, "0.7": 0.7, "1.0": 1.0}
P_PREV = [0.2, 0.0, 0.8]
NORM_M = [0, 2, 1, 0, 0, 2, 1, 2, 2, 0, 1, 2]
NORM_W = [0.3, 1.7, 2.5e-3, 0.11, 4.0, 0.9, 7.5e-3, 0.25, 3.1, 0.6, 1e-4, 0.05]


class _History:
    def get_model_probabilities(self, t):
        return pd.DataFrame({"p": P_PREV}, index=[0, 1, 2])


class _Unit:
    def pdf(self, x):
        return 1.0


def gen():
    res = {"P_PREV": np.array(P_PREV)}
    for tag, stay in STAYS.items():
        for M in (1, 2, 5):
            k = ModelPerturbationKernel(M, probability_to_stay=stay)
            res[f"pmf_M{M}_stay{tag}"] = np.array(
                [[float(k.pmf(n, m)) for m in range(M)] for n in range(M + 1)])
        abc = object.__new__(ABCSMC)
        abc.history = _History()
        abc.model_perturbation_kernel = ModelPerturbationKernel(3, probability_to_stay=stay)
        abc.transitions = [_Unit()] * 3
        pdf = abc._create_transition_pdf(1)
        res[f"factor_stay{tag}"] = np.array([float(pdf(m, {"a": 0.0})) for m in range(3)])
    parts = [Particle(m=m, parameter=Parameter(a=float(i)), weight=w,
                      accepted_sum_stats=[{"y": 0.0}], accepted_distances=[float(i)])
             for i, (m, w) in enumerate(zip(NORM_M, NORM_W))]
    pop = Population(parts)
    res["NORM_m"], res["NORM_w"] = np.array(NORM_M), np.array(NORM_W)
    res["NORM_w_out"] = np.array([p.weight for p in pop.get_list()])
    mp = pop.get_model_probabilities()
    res["NORM_p"] = np.array([mp[m] for m in range(3)])
    res["NORM_wd"] = np.asarray(pop.get_weighted_distances()["w"], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "models.npz"), **res)
    print("models", len(res), "arrays")


if __name__ == "__main__":
    gen()
