# Adapted from pyABC (https://github.com/ICB-DCM/pyABC), BSD-3-Clause,
# Copyright 2017 the pyABC developers -- see NOTICE at the repository root.
"""The distances with a measure list.

Reference: pyabc/distance/distance.py
  DistanceWithMeasureList   :634-664
  ZScoreDistance            :667-686
  PCADistance               :689-739
  RangeEstimatorDistance    :742-834
  MinMaxDistance            :837-849
  PercentileDistance        :852-873
Constructors, attributes, ``initialize``, ``__call__`` and ``get_config`` are
the reference's; ``__call__`` is its per-key arithmetic on the host in
float64 (the per-particle path, no device).

ZScoreDistance and the range distances are weighted 1-norms: with
``weight_vector`` (1 / normalization, or 1 / (|x_0| n) for the z-score, 0 for
a key outside ``measures_to_use``) they provide ``device_call`` (abc_pnorm
with p = 1) and ``fused_pnorm``, so BatchedGPUSampler runs them through the
fused candidate round and abc_pnorm_accept.  From a ``SumStatMatrix``
MinMaxDistance normalizes with abc_column_span and PercentileDistance with
abc_column_quantile.

PCADistance's whitening matrix comes from the centred Gram matrix
(abc_column_gram from a ``SumStatMatrix``, numpy otherwise) through
scipy.linalg.eigh on the host; its batch forms are abc_whitened_norm and the
staged round's accept tail abc_whitened_accept (S <= 256).

A user's own subclass of DistanceWithMeasureList has no device form and keeps
the per-candidate loop.
"""
import numpy as np
import scipy.linalg as la

from .. import gpu
from .base import Distance
from .distance import SumStatMatrix


class DistanceWithMeasureList(Distance):
    def __init__(self, measures_to_use='all'):
        super().__init__()
        # the measures (summary statistics) to use for distance calculation
        self.measures_to_use = measures_to_use

    def initialize(self, t, get_all_sum_stats, x_0=None):
        if self.measures_to_use == 'all':
            self.measures_to_use = list(x_0.keys())

    def get_config(self):
        config = super().get_config()
        config["measures_to_use"] = self.measures_to_use
        return config

    def __getstate__(self):
        state = self.__dict__.copy()
        if "_dev_cache" in state:
            state["_dev_cache"] = {}     # device tensors stay per process
        return state

    def _cached_dev(self, arr, device):
        """arr on the device, uploaded only when its content changed (as
        PNormDistance._device_weights)."""
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        key = (arr.tobytes(), arr.shape, str(device))
        cache = self.__dict__.setdefault("_dev_cache", {})
        if key not in cache:
            cache.clear()
            cache[key] = gpu.as_dev(arr, device=device)
        return cache[key]

    def _matrix_in_key_order(self, sum_stats, x_0):
        """The device matrix of a SumStatMatrix whose columns are x_0's keys
        in order (and a device form exists for them), else None."""
        if isinstance(sum_stats, SumStatMatrix) and x_0 is not None \
                and sum_stats.keys == list(x_0.keys()) and len(sum_stats) > 0:
            return sum_stats.data
        return None


class _WeightedOneNorm:
    """Device forms of a distance sum_k |w_k (x_k - x_0k)| given its
    ``weight_vector``; ``_host_call`` names the class whose ``__call__`` that
    is (a subclass with its own ``__call__`` keeps the per-candidate loop)."""

    _host_call = None

    @property
    def batched_why_not(self):
        if type(self).__call__ is not self._host_call.__call__:
            return f"{type(self).__name__} replaces {self._host_call.__name__}.__call__"
        return ""

    @property
    def batched_capable(self):
        return not self.batched_why_not

    def _device_weights(self, t, keys, device):
        return self._cached_dev(self.weight_vector(t, keys), device)

    def device_call(self, xmat, x0vec, t, keys, out=None):
        """Distances of B simulations (device [B, S], columns in ``keys``
        order) to x_0 (device [S])."""
        return gpu.pnorm(xmat, x0vec, self._device_weights(t, keys, xmat.device),
                         1.0, out=out)

    def fused_pnorm(self, t, keys, device):
        """(weights device [S], p = 1) for the fused candidate kernel and the
        accept tail."""
        if self.batched_why_not:
            return None
        return self._device_weights(t, keys, device), 1.0


class ZScoreDistance(_WeightedOneNorm, DistanceWithMeasureList):
    def __init__(self, measures_to_use='all'):
        super().__init__(measures_to_use)
        self.x_0 = None

    def initialize(self, t, get_all_sum_stats, x_0=None):
        super().initialize(t, get_all_sum_stats, x_0)
        self.x_0 = x_0

    @property
    def batched_why_not(self):
        # x == x_0 == 0 is 0 and x != x_0 == 0 is inf in the reference: no
        # weight expresses both
        if self.x_0 is not None and self.measures_to_use != 'all' and \
                any(self.x_0[key] == 0 for key in self.measures_to_use):
            return "ZScoreDistance with a zero observation"
        return super().batched_why_not

    def weight_vector(self, t, keys):
        """1 / (|x_0[key]| n_measures) per key (x_0 order), 0 for a key
        outside measures_to_use."""
        n = len(self.measures_to_use)
        use = set(self.measures_to_use)
        with np.errstate(divide="ignore"):
            return np.array([np.float64(1.0) / (np.abs(np.float64(self.x_0[k])) * n)
                             if k in use else 0.0 for k in keys], dtype=np.float64)

    def __call__(self, x, x_0, t=None, par=None):
        return sum(abs((x[key] - x_0[key]) / x_0[key]) if x_0[key] != 0 else
                   (0 if x[key] == 0 else np.inf)
                   for key in self.measures_to_use) / len(self.measures_to_use)


ZScoreDistance._host_call = ZScoreDistance


class PCADistance(DistanceWithMeasureList):
    MAX_DEVICE_STATS = 256      # abc_whitened_norm, abc_column_gram

    def __init__(self, measures_to_use='all'):
        super().__init__(measures_to_use)
        self._whitening_transformation_matrix = None
        self._n_stats = None

    def _dict_to_vect(self, x):
        return np.asarray([x[key] for key in self.measures_to_use])

    def _whiten(self, covariance):
        # distance.py:716-718, unguarded: a non-positive eigenvalue gives the
        # reference's non-finite matrix
        w, v = la.eigh(covariance)
        with np.errstate(divide="ignore", invalid="ignore"):
            self._whitening_transformation_matrix = (
                v.dot(np.diag(1. / np.sqrt(w))).dot(v.T))

    def _calculate_whitening_transformation_matrix(self, sum_stats):
        samples_vec = np.asarray([self._dict_to_vect(x)
                                  for x in sum_stats])
        # samples_vec is an array of shape nr_samples x nr_features
        means = samples_vec.mean(axis=0)
        centered = samples_vec - means
        self._whiten(centered.T.dot(centered))

    def initialize(self, t, get_all_sum_stats, x_0=None):
        super().initialize(t, get_all_sum_stats, x_0)
        self._n_stats = None if x_0 is None else len(x_0)
        all_sum_stats = get_all_sum_stats()
        mat = self._matrix_in_key_order(all_sum_stats, x_0)
        if mat is None or mat.shape[1] > self.MAX_DEVICE_STATS:
            self._calculate_whitening_transformation_matrix(all_sum_stats)
            return
        # the centred Gram matrix of all columns on the device; the chosen
        # ones' block is the reference's covariance
        keys = list(x_0.keys())
        cols = [keys.index(key) for key in self.measures_to_use]
        G = gpu.column_gram(mat)[1].cpu().numpy()
        self._whiten(G[np.ix_(cols, cols)])

    def __call__(self, x, x_0, t=None, par=None):
        x_vec, x_0_vec = self._dict_to_vect(x), self._dict_to_vect(x_0)
        distance = la.norm(
            self._whitening_transformation_matrix.dot(x_vec - x_0_vec), 2)
        return distance

    # -- device form ---------------------------------------------------------
    @property
    def batched_why_not(self):
        if type(self).__call__ is not PCADistance.__call__:
            return f"{type(self).__name__} replaces PCADistance.__call__"
        if self._n_stats is not None and self._n_stats > self.MAX_DEVICE_STATS:
            return (f"PCADistance over {self._n_stats} summary statistics (the "
                    f"device kernel takes {self.MAX_DEVICE_STATS})")
        return ""

    @property
    def batched_capable(self):
        return not self.batched_why_not

    def whitening_matrix(self, keys):
        """W embedded into [S x S] over ``keys`` (x_0 order): zero rows and
        columns for the keys outside measures_to_use."""
        keys = list(keys)
        cols = [keys.index(key) for key in self.measures_to_use]
        W = np.zeros((len(keys), len(keys)), dtype=np.float64)
        W[np.ix_(cols, cols)] = self._whitening_transformation_matrix
        return W

    def _device_matrix(self, keys, device):
        return self._cached_dev(self.whitening_matrix(keys), device)

    def device_call(self, xmat, x0vec, t, keys, out=None):
        """Distances of B simulations (device [B, S], columns in ``keys``
        order) to x_0 (device [S])."""
        return gpu.whitened_norm(xmat, x0vec, self._device_matrix(keys, xmat.device),
                                 out=out)

    def accept_tail(self, t, keys, device):
        """The staged sampler's accept tail (gpu.WhitenedTail)."""
        return gpu.WhitenedTail(self._device_matrix(keys, device))


class RangeEstimatorDistance(_WeightedOneNorm, DistanceWithMeasureList):
    @staticmethod
    def lower(parameter_list):
        """The lower margin of the range of a list of values."""

    @staticmethod
    def upper(parameter_list):
        """The upper margin of the range of a list of values."""

    def __init__(self, measures_to_use='all'):
        super().__init__(measures_to_use)
        self.normalization = None

    def get_config(self):
        config = super().get_config()
        config["normalization"] = self.normalization
        return config

    def _calculate_normalization(self, sum_stats):
        measures = {name: [] for name in self.measures_to_use}
        for sample in sum_stats:
            for measure in self.measures_to_use:
                measures[measure].append(sample[measure])
        self.normalization = {measure:
                              self.upper(measures[measure])
                              - self.lower(measures[measure])
                              for measure in self.measures_to_use}

    def _device_range(self, mat):
        """upper - lower of every column of the device matrix (host array),
        or None when this class has no kernel for its margins."""
        return None

    def initialize(self, t, get_all_sum_stats, x_0=None):
        super().initialize(t, get_all_sum_stats, x_0)
        all_sum_stats = get_all_sum_stats()
        mat = self._matrix_in_key_order(all_sum_stats, x_0)
        span = None if mat is None else self._device_range(mat)
        if span is None:
            self._calculate_normalization(all_sum_stats)
            return
        keys = list(x_0.keys())
        self.normalization = {measure: span[keys.index(measure)]
                              for measure in self.measures_to_use}

    def weight_vector(self, t, keys):
        """1 / normalization[key] per key (x_0 order), 0 for a key outside
        measures_to_use; a zero normalization gives inf (the reference's
        division by zero under IEEE)."""
        with np.errstate(divide="ignore"):
            return np.array([np.float64(1.0) / np.float64(self.normalization[k])
                             if k in self.normalization else 0.0 for k in keys],
                            dtype=np.float64)

    def __call__(self, x, x_0, t=None, par=None):
        distance = sum(abs((x[key] - x_0[key]) / self.normalization[key])
                       for key in self.measures_to_use)
        return distance


RangeEstimatorDistance._host_call = RangeEstimatorDistance


class MinMaxDistance(RangeEstimatorDistance):
    @staticmethod
    def upper(parameter_list):
        return max(parameter_list)

    @staticmethod
    def lower(parameter_list):
        return min(parameter_list)

    def _device_range(self, mat):
        # max - min, exact (abc_column_span); a subclass with margins of its
        # own keeps the host loop
        cls = type(self)
        if cls.upper is not MinMaxDistance.upper or cls.lower is not MinMaxDistance.lower \
                or mat.shape[1] > 256:
            return None
        return gpu.column_span(mat).cpu().numpy()


class PercentileDistance(RangeEstimatorDistance):
    PERCENTILE = 20  #: The percentiles

    @staticmethod
    def upper(parameter_list):
        return np.percentile(parameter_list,
                             100 - PercentileDistance.PERCENTILE)

    @staticmethod
    def lower(parameter_list):
        return np.percentile(parameter_list,
                             PercentileDistance.PERCENTILE)

    def get_config(self):
        config = super().get_config()
        config["PERCENTILE"] = self.PERCENTILE
        return config

    def _device_range(self, mat):
        # np.percentile's q is percent / 100 (abc_column_quantile, twice); the
        # margins read PercentileDistance.PERCENTILE when initialize runs
        cls = type(self)
        if cls.upper is not PercentileDistance.upper or \
                cls.lower is not PercentileDistance.lower:
            return None
        pct = PercentileDistance.PERCENTILE
        upper = gpu.column_quantile(mat, (100 - pct) / 100)
        lower = gpu.column_quantile(mat, pct / 100)
        return upper.cpu().numpy() - lower.cpu().numpy()
