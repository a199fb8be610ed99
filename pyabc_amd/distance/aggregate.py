# Adapted from pyABC (https://github.com/ICB-DCM/pyABC), BSD-3-Clause,
# Copyright 2017 the pyABC developers -- see NOTICE at the repository root.
"""AggregatedDistance / AdaptiveAggregatedDistance.

Reference: pyabc/distance/distance.py
  AggregatedDistance            :366-507 (initialize :411-419, update
                                 :432-443, __call__ :445-461)
  AdaptiveAggregatedDistance    :510-631 (_update :594-625)
The interface is the reference's.  When every child is a plain PNormDistance
(or AdaptivePNormDistance) the children form a term stack -- K p-norms read
from the same row -- and the batch forms run on the device: ``device_call``
(abc_aggregate_distance), the staged sampler's accept tail
(abc_aggregate_accept) and the adaptive update's term matrix with its scale
(abc_column_span / abc_column_scale).  Any other child keeps the reference's
per-candidate evaluation through the child's own ``__call__``.
"""
import logging

import numpy as np

from .. import _native as nat
from .. import gpu
from ..storage.json import save_dict_to_json
from .base import Distance, to_distance
from .distance import PNormDistance, SumStatMatrix
from .scale import mean, median, span

logger = logging.getLogger("Distance")


class AggregatedDistance(Distance):
    def __init__(self, distances, weights=None, factors=None):
        super().__init__()
        if not isinstance(distances, list):
            distances = [distances]
        self.distances = [to_distance(distance) for distance in distances]
        self.weights = weights
        self.factors = factors
        self._dev_stack_cache = {}

    def initialize(self, t, get_all_sum_stats, x_0=None):
        super().initialize(t, get_all_sum_stats, x_0)
        for distance in self.distances:
            distance.initialize(t, get_all_sum_stats, x_0)
        self.format_weights_and_factors(t)

    def configure_sampler(self, sampler):
        for distance in self.distances:
            distance.configure_sampler(sampler)

    def update(self, t, get_all_sum_stats):
        # (a generator, as in distance.py:442-443: children after the first
        # that reports an update are not updated in this call)
        return any(distance.update(t, get_all_sum_stats)
                   for distance in self.distances)

    def __call__(self, x, x_0, t=None, par=None):
        values = np.array([distance(x, x_0, t, par) for distance in self.distances])
        return float(np.dot(self.term_weights(t), values))

    def term_weights(self, t):
        """weights * factors [K] for generation t (distance.py:458-461)."""
        self.format_weights_and_factors(t)
        weights = AggregatedDistance.get_for_t_or_latest(self.weights, t)
        factors = AggregatedDistance.get_for_t_or_latest(self.factors, t)
        return np.asarray(weights, dtype=np.float64) * np.asarray(factors, dtype=np.float64)

    def get_config(self):
        return {f"Distance_{j}": distance.get_config()
                for j, distance in enumerate(self.distances)}

    def format_weights_and_factors(self, t):
        self.weights = AggregatedDistance.format_dict(
            self.weights, t, len(self.distances))
        self.factors = AggregatedDistance.format_dict(
            self.factors, t, len(self.distances))

    @staticmethod
    def format_dict(w, t, n_distances, default_val=1.):
        if w is None:
            w = {t: default_val * np.ones(n_distances)}
        elif not isinstance(w, dict):
            w = {t: np.array(w)}
        return w

    @staticmethod
    def get_for_t_or_latest(w, t):
        if t not in w:
            t = max(w)
        return w[t]

    # -- device form ---------------------------------------------------------
    @property
    def batched_why_not(self):
        """'' when the children form a term stack, else the reason."""
        if len(self.distances) > nat.ABC_AGG_MAX_TERMS:
            return (f"AggregatedDistance of {len(self.distances)} distances "
                    f"(the device kernel takes {nat.ABC_AGG_MAX_TERMS})")
        for j, distance in enumerate(self.distances):
            cls = type(distance)
            # PNormDistance.fused_pnorm's test, without touching the device
            if not isinstance(distance, PNormDistance) or \
                    cls.device_call is not PNormDistance.device_call or \
                    cls.__call__ is not PNormDistance.__call__ or \
                    cls.weight_vector is not PNormDistance.weight_vector:
                return (f"AggregatedDistance child {j} ({cls.__name__}) is "
                        "not a plain PNormDistance")
        return ""

    @property
    def batched_capable(self):
        return not self.batched_why_not

    def term_stack(self, t, keys, device, c=None):
        """The children as a gpu.TermStack for generation t, uploaded only
        when its content changed (as PNormDistance._device_weights)."""
        why = self.batched_why_not
        if why:
            raise TypeError(why)
        keys = list(keys)
        wf = np.ascontiguousarray(
            [distance.weight_vector(t, keys) for distance in self.distances],
            dtype=np.float64)
        pv = np.array([float(distance.p) for distance in self.distances])
        c = self.term_weights(t) if c is None else np.asarray(c, dtype=np.float64)
        if c.shape != pv.shape:
            raise ValueError(f"AggregatedDistance: {c.size} weights * factors "
                             f"for {pv.size} distances")
        key = (wf.tobytes(), pv.tobytes(), c.tobytes(), str(device))
        cache = self.__dict__.setdefault("_dev_stack_cache", {})
        if key not in cache:
            cache.clear()
            cache[key] = gpu.TermStack(gpu.as_dev(wf, device=device), pv, c)
        return cache[key]

    def device_call(self, xmat, x0vec, t, keys, out=None):
        """Aggregated distances of B simulations (device [B, S], columns in
        ``keys`` order) to x_0 (device [S])."""
        return gpu.aggregate_distance(xmat, x0vec,
                                      self.term_stack(t, keys, xmat.device), out=out)

    def accept_tail(self, t, keys, device):
        """The staged sampler's accept tail (gpu.AggregateTail)."""
        return gpu.AggregateTail(self.term_stack(t, keys, device))

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_dev_stack_cache"] = {}     # device tensors stay per process
        return state


class AdaptiveAggregatedDistance(AggregatedDistance):
    def __init__(self, distances, initial_weights=None, factors=None,
                 adaptive=True, scale_function=None, log_file=None):
        super().__init__(distances=distances)
        self.initial_weights = initial_weights
        self.factors = factors
        self.adaptive = adaptive
        self.x_0 = None
        if scale_function is None:
            scale_function = span
        self.scale_function = scale_function
        self.log_file = log_file

    def initialize(self, t, get_all_sum_stats, x_0=None):
        super().initialize(t, get_all_sum_stats, x_0)
        self.x_0 = x_0
        if self.initial_weights is not None:
            self.weights[t] = self.initial_weights
            return
        self._update(t, get_all_sum_stats())

    def update(self, t, get_all_sum_stats):
        super().update(t, get_all_sum_stats)
        if not self.adaptive:
            return False
        self._update(t, get_all_sum_stats())
        return True

    def _term_scales(self, sum_stats):
        """scale_function of every child's distances over the recorded sum
        stats (distance.py:603-610): the children's latest weights (t = None,
        after their own update)."""
        keys = list(self.x_0.keys())
        if isinstance(sum_stats, SumStatMatrix) and sum_stats.keys == keys \
                and len(sum_stats) > 0 and self.batched_capable:
            mat = sum_stats.data
            x0 = gpu.as_dev(np.array([float(self.x_0[k]) for k in keys]),
                            device=mat.device)
            stack = self.term_stack(None, keys, mat.device,
                                    c=np.ones(len(self.distances)))
            _, terms = gpu.aggregate_distance(mat, x0, stack, terms=True)
            # by identity: the three functions carry no device_kernel tag
            if self.scale_function is span:
                return gpu.column_span(terms).cpu().numpy()
            if self.scale_function is mean or self.scale_function is median:
                # terms are >= 0: their mean / median is the mean / median
                # absolute deviation to a zero observation
                kind = (nat.ABC_SCALE_MEAN_AD_TO_OBS if self.scale_function is mean
                        else nat.ABC_SCALE_MAD_TO_OBS)
                zero = gpu.torch.zeros(terms.shape[1], dtype=gpu.F64, device=mat.device)
                return gpu.column_scale(terms, kind, zero).cpu().numpy()
            cols = terms.cpu().numpy()
            return np.array([self.scale_function(cols[:, j].tolist())
                             for j in range(cols.shape[1])], dtype=np.float64)
        return np.array([
            self.scale_function([distance(sum_stat, self.x_0) for sum_stat in sum_stats])
            for distance in self.distances], dtype=np.float64)

    def _update(self, t, sum_stats):
        scales = self._term_scales(sum_stats)
        # distance.py:612-619: the inverted scale, 0 for a vanishing one
        w = [0 if np.isclose(scale, 0) else 1 / scale for scale in scales]
        self.weights[t] = np.array(w)
        self.log(t)

    def log(self, t):
        logger.debug("updated weights[%s] = %s", t, self.weights[t])
        if self.log_file:
            save_dict_to_json(self.weights, self.log_file)
