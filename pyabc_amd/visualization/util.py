"""Helpers shared by the plot functions."""


def format_plot_matrix(arr_ax, par_names):
    """The axis-matrix formatting of pyabc/visualization/util.py:23-55: no
    inner labels or legends, no top / right spines, the parameter names along
    the bottom row and the left column."""
    n = len(par_names)
    for i in range(n):
        for j in range(n):
            ax = arr_ax[i, j]
            ax.set_xlabel("")
            ax.set_ylabel("")
            ax.legend = None
            ax.spines["right"].set_visible(False)
            ax.spines["top"].set_visible(False)
    for k, name in enumerate(par_names):
        arr_ax[n - 1, k].set_xlabel(name)
        arr_ax[k, 0].set_ylabel(name)
