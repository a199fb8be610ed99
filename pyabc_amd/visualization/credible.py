"""Credible intervals of the parameters over the generations.

Behaviour as documented for pyabc.visualization's ``plot_credible_intervals``,
``compute_credible_interval``, ``compute_quantile`` and ``compute_kde_max``.
The quantiles go through the device weighted-quantile select
(``gpu.weighted_quantile``); the MAP marker (``compute_kde_max``) is the
estimator's device fit and its density at every particle, N x N, in one
kernel call instead of a Python loop over the rows.  The numbers behind the
plot are gathered per generation by ``interval_table`` and drawn per
parameter by ``_draw_parameter``; matplotlib is imported inside
``plot_credible_intervals`` only.
"""
import numpy as np

from .. import gpu
from ..transition.multivariatenormal import MultivariateNormalTransition
from .kde import DevicePopulation


def _dev(a):
    if gpu.torch is not None and isinstance(a, gpu.torch.Tensor):
        return a.to(dtype=gpu.F64).contiguous()
    gpu.require_device()
    return gpu.as_dev(np.asarray(a, dtype=np.float64).ravel())


def compute_quantile(vals, weights, alpha):
    """The alpha-quantile of the points vals under the (normalised) weights,
    as ``weighted_statistics.weighted_quantile``.  vals and weights: numpy
    arrays or device tensors."""
    v, w = _dev(vals), _dev(weights)
    s = float(w.sum())
    if not np.isclose(s, 1):
        raise AssertionError(f"Weights not normalized: {s}.")
    q = gpu.weighted_quantile(v, w, alpha)
    return gpu.resolve_quantile(q.cpu()[0], v, w, alpha)


def _tail(confidence):
    """Mass left below a central interval of that level; checks the level."""
    if not 0.0 < confidence < 1.0:
        raise ValueError(
            f"Confidence {confidence} must be in the interval (0.0, 1.0).")
    return 0.5 * (1.0 - confidence)


def compute_credible_interval(vals, weights, confidence=0.95):
    """(lower, upper) bound of the central credible interval at that level."""
    tail = _tail(confidence)
    return (compute_quantile(vals, weights, tail),
            compute_quantile(vals, weights, confidence + tail))


def kde_max_index(kde, df, w=None):
    """Row of the population at which the fitted kde is largest: the lowest
    index among the maxima (what a first-match search for the maximum of the
    per-row densities gives).  Returns (index, the DevicePopulation)."""
    pop = DevicePopulation(df, w)
    if hasattr(kde, "fit_device") and hasattr(kde, "logpdf_device"):
        kde.fit_device(pop.X, pop.w, pop.names)
        lp = kde.logpdf_device(pop.X)
        top = gpu.torch.nonzero(lp == lp.max())
        # no row equals a NaN maximum: the first row, as a max() over NaNs
        return (int(top[0, 0].cpu()) if top.numel() else 0), pop
    kde.fit(pop.frame(), pop.weights().copy())
    dens = np.array([kde.pdf(row) for _, row in pop.frame().iterrows()])
    return (0 if np.isnan(dens).all() else int(np.nanargmax(dens))), pop


def compute_kde_max(kde, df, w=None):
    """Fit the kde and return the particle (a Series over the parameter names)
    at which its density is highest among the particles."""
    ix, pop = kde_max_index(kde, df, w)
    return pop.row(ix)


def interval_table(history, m=0, ts=None, par_names=None, levels=(0.95,),
                   mean=False, kde=None, kde_1d=None):
    """The numbers behind plot_credible_intervals: {parameter: {"median" [T],
    "lower" [L, T], "upper" [L, T], and where asked for "mean" [T] (mean=True),
    "kde_max" [T] (an estimator as kde: the MAP particle of the joint KDE) and
    "kde_max_1d" [T] (an estimator as kde_1d: of the parameter's own 1-D
    KDE)}} over the generations ts and the levels, in the order given."""
    ts = list(ts)
    levels = list(levels)
    tails = [_tail(c) for c in levels]
    table = None
    for col, t in enumerate(ts):
        pop = DevicePopulation.of_history(history, m, t)
        names = pop.names if par_names is None else list(par_names)
        if table is None:
            table = {n: dict(median=np.empty(len(ts)),
                             lower=np.empty((len(levels), len(ts))),
                             upper=np.empty((len(levels), len(ts))))
                     for n in names}
        top = compute_kde_max(kde, pop) if kde is not None else None
        for n in names:
            vals, out = pop.column(n), table[n]
            out["median"][col] = compute_quantile(vals, pop.w, 0.5)
            for row, (c, tail) in enumerate(zip(levels, tails)):
                out["lower"][row, col] = compute_quantile(vals, pop.w, tail)
                out["upper"][row, col] = compute_quantile(vals, pop.w, c + tail)
            if mean:
                out.setdefault("mean", np.empty(len(ts)))[col] = float((pop.w * vals).sum())
            if top is not None:
                out.setdefault("kde_max", np.empty(len(ts)))[col] = top[n]
            if kde_1d is not None:
                own = compute_kde_max(kde_1d, pop.select([n]))
                out.setdefault("kde_max_1d", np.empty(len(ts)))[col] = own[n]
    return table or {}


_MARKS = (("mean", "Mean"), ("kde_max", "Max KDE"), ("kde_max_1d", "Max KDE 1d"))


def _draw_parameter(ax, name, ts, stats, levels, refval, refval_color):
    """One parameter's axis: the median with one error bar per level (widest
    level first so the narrower ones lie on top, caps widening with the
    level), the optional markers, the reference line, ticks at the
    generations."""
    pos = np.arange(len(ts))
    med = stats["median"]
    order = np.argsort(levels)                       # rank 0 = narrowest
    for rank in range(len(levels) - 1, -1, -1):
        k = order[rank]
        ax.errorbar(pos, med, yerr=np.stack([med - stats["lower"][k],
                                             stats["upper"][k] - med]),
                    capsize=5.0 * (rank + 1) / len(levels), label=f"{levels[k]:.2f}")
    for key, label in _MARKS:
        if key in stats:
            ax.plot(pos, stats[key], "x-", label=label)
    if refval is not None:
        ax.hlines(refval[name], xmin=0, xmax=len(ts) - 1, color=refval_color,
                  label="Reference value")
    ax.set_title(f"Parameter {name}")
    ax.set_ylabel(name)
    ax.set_xticks(pos)
    ax.set_xticklabels(ts)
    ax.legend()


def plot_credible_intervals(history, m=0, ts=None, par_names=None, levels=None,
                            show_mean=False, show_kde_max=False,
                            show_kde_max_1d=False, size=None, refval=None,
                            refval_color="C1", kde=None, kde_1d=None,
                            arr_ax=None):
    """Median and central credible intervals of every parameter of model m
    over the generations ts (default: all), one axis per parameter.

    levels: the interval levels (default [0.95]).  show_mean adds the weighted
    mean; show_kde_max the particle of highest density under ``kde`` (default
    a MultivariateNormalTransition) fitted to the generation, show_kde_max_1d
    the same per parameter under ``kde_1d``.  refval {name: value} draws a
    horizontal reference line.  arr_ax: a 1-D list of axes to draw into.
    Returns the list (or array) of axes."""
    import matplotlib.pyplot as plt
    if ts is None:
        ts = range(history.max_t + 1)
    ts = [int(ts)] if isinstance(ts, (int, np.integer)) else list(ts)
    if par_names is None:
        par_names = list(history.get_distribution(m=m)[0].columns)
    levels = [0.95] if levels is None else list(levels)
    if show_kde_max and kde is None:
        kde = MultivariateNormalTransition()
    if show_kde_max_1d and kde_1d is None:
        kde_1d = MultivariateNormalTransition()
    table = interval_table(history, m, ts, par_names, levels, mean=show_mean,
                           kde=kde if show_kde_max else None,
                           kde_1d=kde_1d if show_kde_max_1d else None)
    if arr_ax is None:
        _, arr_ax = plt.subplots(nrows=len(par_names), ncols=1, figsize=size)
    if not isinstance(arr_ax, (list, np.ndarray)):
        arr_ax = [arr_ax]
    for ax, name in zip(arr_ax, par_names):
        _draw_parameter(ax, name, ts, table[name], levels, refval, refval_color)
    arr_ax[-1].set_xlabel("Population t")
    fig = arr_ax[0].get_figure()
    if size is not None:
        fig.set_size_inches(size)
    fig.tight_layout()
    return arr_ax
