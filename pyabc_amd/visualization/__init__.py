"""Posterior KDE plots and credible intervals (pyabc.visualization's KDE and
credible-interval family), evaluated on the population in HBM.

Not here: the histogram, epsilon, sample-number, effective-sample-size and
model-probability plots, ``plot_credible_intervals_for_time`` and the data
plots -- table plots over ``History`` with no kernel behind them.
"""
from .kde import (kde_1d, kde_2d, kde_matrix, plan_panels, matrix_pairs, route,
                  KdeMatrix, PanelPlan, DevicePopulation, plot_kde_1d,
                  plot_kde_1d_highlevel, plot_kde_2d, plot_kde_2d_highlevel,
                  plot_kde_matrix, plot_kde_matrix_highlevel)
from .credible import (compute_quantile, compute_credible_interval,
                       compute_kde_max, kde_max_index, interval_table,
                       plot_credible_intervals)
from .util import format_plot_matrix
