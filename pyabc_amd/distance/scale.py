"""Scale functions for AdaptivePNormDistance (pyabc/distance/scale.py).

The ten sum-stat scale functions (scale.py:38-135) carry a ``device_kernel``
tag: the adaptive distance evaluates them on the GPU over the recorded
[R x S] sum-stat matrix, all columns in one call (abc_column_std /
abc_column_mad for ``standard_deviation`` / ``median_absolute_deviation``,
abc_column_scale for the others; the tags are the keys of
``_native.SCALE_KINDS``).  Called on a plain list (the reference signature
``f(data=list, x_0=float)``) ``standard_deviation`` and
``median_absolute_deviation`` evaluate one column through the same kernels
and the other eight are the reference's numpy expressions.  ``span``,
``mean`` and ``median`` (scales of the reference's AdaptiveAggregatedDistance)
are untagged host functions.
"""
import numpy as np


def _column(data):
    from .. import gpu
    return gpu.as_dev(np.asarray(data, dtype=np.float64).reshape(-1, 1))


def median_absolute_deviation(data, **kwargs):
    """scale.py:38-47: median(|x - median(x)|)."""
    from .. import gpu
    return float(gpu.column_mad(_column(data)).cpu()[0])


median_absolute_deviation.device_kernel = "mad"


def standard_deviation(data, **kwargs):
    """scale.py:59-65: np.std."""
    from .. import gpu
    return float(gpu.column_std(_column(data)).cpu()[0])


standard_deviation.device_kernel = "std"


def mean_absolute_deviation(data, **kwargs):
    data = np.array(data)
    return np.mean(np.abs(data - np.mean(data)))


mean_absolute_deviation.device_kernel = "mean_ad"


def bias(data, x_0, **kwargs):
    return np.abs(np.mean(data) - x_0)


bias.device_kernel = "bias"


def root_mean_square_deviation(data, x_0, **kwargs):
    return np.sqrt(bias(data, x_0) ** 2 + np.std(data) ** 2)


root_mean_square_deviation.device_kernel = "rmsd"


def median_absolute_deviation_to_observation(data, x_0, **kwargs):
    return np.median(np.abs(np.array(data) - x_0))


median_absolute_deviation_to_observation.device_kernel = "mad_to_obs"


def mean_absolute_deviation_to_observation(data, x_0, **kwargs):
    return np.mean(np.abs(np.array(data) - x_0))


mean_absolute_deviation_to_observation.device_kernel = "mean_ad_to_obs"


def combined_median_absolute_deviation(data, x_0, **kwargs):
    # the MAD in numpy like its other half (the same bits as the select
    # kernel's: both are exact order statistics)
    data = np.array(data)
    return (np.median(np.abs(data - np.median(data)))
            + median_absolute_deviation_to_observation(data, x_0))


combined_median_absolute_deviation.device_kernel = "cmad"


def combined_mean_absolute_deviation(data, x_0, **kwargs):
    return (mean_absolute_deviation(data)
            + mean_absolute_deviation_to_observation(data, x_0))


combined_mean_absolute_deviation.device_kernel = "cmean_ad"


def standard_deviation_to_observation(data, x_0, **kwargs):
    return np.std(np.abs(np.array(data) - x_0))


standard_deviation_to_observation.device_kernel = "std_to_obs"


def span(data, **kwargs):
    return max(data) - min(data)


def mean(data, **kwargs):
    return np.mean(data)


def median(data, **kwargs):
    return np.median(data)
