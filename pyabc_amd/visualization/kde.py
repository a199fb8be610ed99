"""Kernel density estimates of a weighted population on plot grids.

Reference: pyabc/visualization/kde.py.  ``kde_1d`` / ``kde_2d`` fit a
transition to one or two columns and evaluate its pdf on a ``linspace`` /
``meshgrid`` grid; ``plot_kde_matrix`` does that for every parameter and
every pair.  Here all panels of one call are planned from a single moments
pass (every panel's covariance is a sub-block of the one d x d weighted
covariance) and evaluated by one ``abc_kde_panels`` call on the population
where it already lies, in HBM.

Routes (``route(kde, ...)`` tells which one a call takes):

* ``"device"``: ``kde`` is None or a ``MultivariateNormalTransition`` with
  one of the two built-in bandwidth rules (any ``scaling``), within the
  entry's caps (d <= 64, axes <= 4096 points, 2^24 grid points in all).  One
  ``gpu.weighted_moments``, one ``plan_panels``, one ``gpu.kde_panels`` for all
  regular panels.  Irregular panels (rank-deficient covariance, N = 1) go
  through a fresh estimator's own ``fit`` + ``pdf``, one at a time.  The
  ``kde`` object passed in is left unfitted (the reference leaves it fitted
  to the last panel).
* ``"generic"``: anything else; the estimator's own ``fit`` / ``pdf`` per
  panel, as the reference does.

``df`` / ``w`` are a DataFrame and weights (uploaded once) or the device
columns of a ``History`` (``History.get_population_device``; ``w`` may then be
None).  matplotlib is imported inside the plot functions only.
"""
import numpy as np
import pandas as pd

from .. import gpu
from .. import _native as nat
from ..transition.multivariatenormal import (
    MultivariateNormalTransition, _bw_rule, psd_whitening,
    scott_rule_of_thumb, silverman_rule_of_thumb)
from .util import format_plot_matrix

_BW = {0: silverman_rule_of_thumb, 1: scott_rule_of_thumb}


# ---- planning (pure numpy) -------------------------------------------------

class PanelPlan:
    """plan_panels' result: ``panels`` (one dict per requested panel, in
    request order) and ``coords`` (the axis coordinates of the regular panels,
    concatenated).  A panel dict holds key (the name tuple), cols, axes (the
    linspace arrays), cov (the scaled KDE covariance), bw, irregular, and for
    a regular panel centre, U, log_const, axis (offsets into coords), out."""

    def __init__(self, panels, coords):
        self.panels = panels
        self.coords = coords

    @property
    def regular(self):
        return [q for q in self.panels if not q["irregular"]]

    @property
    def n_points(self):
        return sum(int(np.prod(q["num"])) for q in self.regular)

    def descriptors(self):
        """ctypes array of abc_kde_panel for the regular panels."""
        reg = self.regular
        arr = (nat.KdePanel * len(reg))()
        for a, q in zip(arr, reg):
            two = len(q["cols"]) == 2
            a.col[0], a.col[1] = q["cols"][0], (q["cols"][1] if two else -1)
            a.num[0], a.num[1] = q["num"]
            a.axis[0], a.axis[1] = q["axis"]
            a.centre[0], a.centre[1] = q["centre"]
            U = np.zeros(4)
            U[:q["U"].size] = q["U"].ravel()
            for k in range(4):
                a.U[k] = U[k]
            a.log_const = q["log_const"]
            a.out = q["out"]
        return arr


def matrix_pairs(names):
    """The panels of the KDE matrix in its drawing order: per row i the 1-D
    panel (names[i],), then the pairs (names[j], names[i]) for j < i."""
    pairs = []
    for i, yn in enumerate(names):
        pairs.append((yn,))
        pairs.extend((xn, yn) for xn in names[:i])
    return pairs


def plan_panels(names, cov, ess, lo, hi, limits=None, numx=50, numy=50,
                scaling=1.0, bw_rule=0, pairs=None, mean=None, n_particles=None):
    """Descriptors of the requested panels from one weighted covariance.

    names [d]; cov [d, d] the weighted sample covariance
    (``np.cov(X.T, aweights=w)``); ess = 1 / sum w^2; lo / hi [d] the column
    minima / maxima; limits {name: (lower, upper)} (either may be None);
    bw_rule 0 (Silverman), 1 (Scott) or a callable (ess, dim); pairs a list of
    (x,) and (x, y) name tuples (default: the KDE matrix: every name, and
    (names[j], names[i]) for j < i); mean [d] the centre subtracted before
    whitening (default: the middle of lo and hi); n_particles: N, when known.

    A panel is irregular, and is not sent to the kernel, when its scaled
    covariance is rank-deficient under ``psd_whitening`` (a constant column,
    two perfectly dependent columns) or when N == 1 (``smart_cov``'s special
    case, which is not a sub-block of anything).
    """
    names = list(names)
    d = len(names)
    cov = np.atleast_2d(np.asarray(cov, dtype=np.float64))
    lo = np.asarray(lo, dtype=np.float64).ravel()
    hi = np.asarray(hi, dtype=np.float64).ravel()
    centre = 0.5 * (lo + hi) if mean is None else np.asarray(mean, dtype=np.float64).ravel()
    limits = {} if limits is None else limits
    if pairs is None:
        pairs = matrix_pairs(names)
    bw_fn = _BW.get(bw_rule, bw_rule)
    panels, coords, n_coords, out = [], [], 0, 0
    for key in pairs:
        key = tuple(key)
        cols = [names.index(k) for k in key]
        k = len(cols)
        if k not in (1, 2):
            raise ValueError(f"plan_panels: a panel has one or two columns, not {key}")
        num = (int(numx), int(numy) if k == 2 else 1)
        axes = []
        for c, n in zip(cols, num):
            a, b = limits.get(names[c], (None, None))
            axes.append(np.linspace(lo[c] if a is None else a,
                                    hi[c] if b is None else b, num=n))
        bw = float(bw_fn(ess, k))
        sub = cov[np.ix_(cols, cols)] * bw ** 2 * scaling
        for a, c in enumerate(cols):
            if lo[c] == hi[c]:
                # a constant column: its moments are the rounding of the
                # weighted mean (~(eps |x|)^2), its variance is 0
                sub[a, :] = 0.0
                sub[:, a] = 0.0
        q = dict(key=key, cols=cols, num=num, axes=axes, cov=sub, bw=bw,
                 irregular=True)
        ok = n_particles != 1 and np.all(np.isfinite(sub))
        if ok:
            psd = psd_whitening(sub)
            ok = psd["rank"] == k
        if ok:
            q.update(irregular=False, U=psd["U"],
                     centre=(centre[cols[0]], centre[cols[1]] if k == 2 else 0.0),
                     log_const=-0.5 * (k * gpu.LOG_2PI + psd["log_pdet"]),
                     out=out)
            offs = []
            for a in axes:
                offs.append(n_coords)
                coords.append(a)
                n_coords += a.size
            q["axis"] = (offs[0], offs[1] if k == 2 else 0)
            out += num[0] * num[1]
        panels.append(q)
    return PanelPlan(panels, np.concatenate(coords) if coords else np.zeros(0))


# ---- the population a call works on ------------------------------------------

class DevicePopulation:
    """The population a call works on: names, device X [N, d] and w [N]
    (normalised), the host frame and weights on demand.  Built from a
    DataFrame and weights, from the device columns of a History (w may then
    be None), or from another DevicePopulation (shared, nothing copied)."""

    def __init__(self, df, w=None):
        if isinstance(df, DevicePopulation):
            self.__dict__.update(df.__dict__)
            return
        if hasattr(df, "theta") and hasattr(df, "param_names"):   # device columns
            self.names = list(df.param_names)
            self.X = df.theta.contiguous()
            wd = df.weights if w is None else w
            self.w = gpu.as_dev(wd, device=self.X.device)
            self._df = self._wh = None
        else:
            if w is None:
                raise ValueError("a DataFrame needs its weights: pass w (only the "
                                 "device columns of a History carry their own)")
            if len(df) == 0:
                from ..transition.exceptions import NotEnoughParticles
                raise NotEnoughParticles("Fitting not possible.")
            gpu.require_device()
            self.names = list(df.columns)
            self._df = df
            self._wh = np.asarray(w, dtype=np.float64)
            self.X = gpu.as_dev(np.asarray(df.values, dtype=np.float64).reshape(len(df), -1))
            self.w = gpu.as_dev(self._wh, device=self.X.device)
        if self.X.shape[0] == 0:
            from ..transition.exceptions import NotEnoughParticles
            raise NotEnoughParticles("Fitting not possible.")
        # TransitionMeta.wrap_fit: weights that do not sum to 1 are normalised
        # (on a copy here: the caller's array stays as it is)
        s = float(self.w.sum())
        if not np.isclose(s, 1):
            self.w = self.w / s
            self._wh = None if self._wh is None else self._wh / self._wh.sum()

    @classmethod
    def of_history(cls, history, m=0, t=None):
        """Generation t of model m: its device columns when resident (of a
        single-model generation only when that model is m), else the host
        frame of ``get_distribution``, which is empty for an absent model."""
        cols = history.get_population_device(t, m)
        if cols is not None and getattr(cols, "theta", None) is not None \
                and len(cols.param_names) > 0 and getattr(cols, "m", m) == m:
            return cls(cols)
        return cls(*history.get_distribution(m=m, t=t))

    def select(self, names):
        """The population of these columns only, on the same rows and weights."""
        sub = DevicePopulation(self)
        sub.names = list(names)
        sub.X = self.X[:, [self.names.index(n) for n in sub.names]].contiguous()
        sub._df = None if self._df is None else self._df[sub.names]
        return sub

    def column(self, name):
        """One column as a contiguous device vector [N]."""
        return self.X[:, self.names.index(name)].contiguous()

    def row(self, i):
        """Row i as a Series over the names (the frame's own row if there is one)."""
        if self._df is not None:
            return self._df.iloc[i]
        return pd.Series(self.X[i].cpu().numpy(), index=self.names, name=i)

    def frame(self):
        if self._df is None:
            self._df = pd.DataFrame(self.X.cpu().numpy(), columns=self.names)
        return self._df

    def weights(self):
        if self._wh is None:
            self._wh = self.w.cpu().numpy()
        return self._wh


def _device_kde(kde):
    return kde is None or (type(kde) is MultivariateNormalTransition and
                           _bw_rule(kde.bandwidth_selector) is not None)


def route(kde=None, d=1, numx=50, numy=50, n_panels=1, n_points=None):
    """The route a call with these arguments takes: "device" or "generic"."""
    if not _device_kde(kde):
        return "generic"
    if n_points is None:
        n_points = n_panels * numx * max(numy, 1)
    ok = (1 <= d <= 64 and 1 <= numx <= nat.ABC_KDE_MAX_AXIS
          and 1 <= numy <= nat.ABC_KDE_MAX_AXIS
          and n_panels <= nat.ABC_KDE_MAX_PANELS
          and n_points <= nat.ABC_KDE_MAX_POINTS)
    return "device" if ok else "generic"


class KdeMatrix(dict):
    """kde_matrix' result: {(name,): (x, pdf), (xname, yname): (X, Y, PDF)},
    with ``route_`` ("device" / "generic") and ``panel_routes_`` {key:
    "kernel" / "estimator"}."""
    route_ = None
    panel_routes_ = None


def _estimator_panel(est, pop, q):
    """One panel through the estimator's own fit + pdf (kde.py:63-74, 231-248)."""
    key = list(q["key"])
    est.fit(pop.frame()[key], pop.weights().copy())
    if len(key) == 1:
        x = q["axes"][0]
        return x, np.asarray(est.pdf(pd.DataFrame({key[0]: x})), dtype=np.float64).reshape(x.shape)
    X, Y = np.meshgrid(q["axes"][0], q["axes"][1])
    pdf = np.asarray(est.pdf(pd.DataFrame({key[0]: X.flatten(), key[1]: Y.flatten()})))
    return X, Y, pdf.reshape(X.shape)


def _panels(pop, pairs, limits, numx, numy, kde):
    d = len(pop.names)
    pairs = matrix_pairs(pop.names) if pairs is None else pairs
    n2 = sum(1 for k in pairs if len(k) == 2)
    res = KdeMatrix()
    res.panel_routes_ = {}
    res.route_ = route(kde, d, numx, numy, len(pairs),
                       n2 * numx * numy + (len(pairs) - n2) * numx)
    lo = pop.X.amin(dim=0).cpu().numpy()
    hi = pop.X.amax(dim=0).cpu().numpy()
    if res.route_ == "generic":
        plan = plan_panels(pop.names, np.full((d, d), np.nan), 1.0, lo, hi, limits,
                           numx, numy, pairs=pairs)
        est = MultivariateNormalTransition(scaling=1) if kde is None else kde
        for q in plan.panels:
            res[q["key"]] = _estimator_panel(est, pop, q)
            res.panel_routes_[q["key"]] = "estimator"
        return res
    scaling = 1 if kde is None else kde.scaling
    rule = 0 if kde is None else _bw_rule(kde.bandwidth_selector)
    N = pop.X.shape[0]
    sw, sw2, mean, cov_b = gpu.weighted_moments(pop.X, pop.w)
    with np.errstate(divide="ignore", invalid="ignore"):
        cov = cov_b * sw / (sw - sw2 / sw)      # np.cov(aweights=w)
    plan = plan_panels(pop.names, cov, 1 / sw2, lo, hi, limits, numx, numy,
                       scaling, rule, pairs, mean=mean, n_particles=N)
    reg = plan.regular
    if reg:
        lp = gpu.kde_panels(pop.X, pop.w, plan.descriptors(), plan.coords)
        dens = gpu.torch.exp(lp).cpu().numpy()
    for q in plan.panels:
        key = q["key"]
        if q["irregular"]:
            est = MultivariateNormalTransition(scaling=scaling, bandwidth_selector=_BW[rule])
            res[key] = _estimator_panel(est, pop, q)
            res.panel_routes_[key] = "estimator"
            continue
        nx, ny = q["num"]
        pdf = dens[q["out"]:q["out"] + nx * ny]
        if len(key) == 1:
            res[key] = (q["axes"][0], pdf.copy())
        else:
            X, Y = np.meshgrid(q["axes"][0], q["axes"][1])
            res[key] = (X, Y, pdf.reshape(X.shape).copy())
        res.panel_routes_[key] = "kernel"
    return res


def _lim(name, lower, upper):
    return {name: (lower, upper)}


def kde_1d(df, w, x, xmin=None, xmax=None, numx=50, kde=None):
    """x values and densities of the 1-D marginal KDE of column x
    (kde.py:19-74): (x_vals [numx], pdf [numx])."""
    return _panels(DevicePopulation(df, w), [(x,)], _lim(x, xmin, xmax), numx, 1, kde)[(x,)]


def kde_2d(df, w, x, y, xmin=None, xmax=None, ymin=None, ymax=None,
           numx=50, numy=50, kde=None):
    """Mesh and densities of the 2-D marginal KDE of columns (x, y)
    (kde.py:174-248): (X, Y, PDF), each [numy, numx]."""
    limits = _lim(x, xmin, xmax)
    limits.update(_lim(y, ymin, ymax))
    return _panels(DevicePopulation(df, w), [(x, y)], limits, numx, numy, kde)[(x, y)]


def kde_matrix(df, w=None, limits=None, numx=50, numy=50, kde=None):
    """The numeric core of plot_kde_matrix: every 1-D marginal and, for
    j < i, the pair (names[j], names[i]) -> KdeMatrix {(name,): (x, pdf),
    (xname, yname): (X, Y, PDF)}.  w may be None only where df carries its own
    weights (device columns, a DevicePopulation)."""
    return _panels(DevicePopulation(df, w), None, limits, numx, numy, kde)


# ---- plots -------------------------------------------------------------------

def _draw_1d(ax, x_vals, pdf, x, xmin, xmax, title, refval, refval_color, size,
             kwargs):
    ax.plot(x_vals, pdf, **kwargs)
    ax.set_xlabel(x)
    ax.set_ylabel("Posterior")
    ax.set_xlim(xmin, xmax)
    if title is not None:
        ax.set_title(title)
    if refval is not None:
        ax.axvline(refval[x], color=refval_color, linestyle="dotted")
    if size is not None:
        ax.get_figure().set_size_inches(size)
    return ax


def _draw_2d(ax, X, Y, PDF, x, y, colorbar, title, refval, refval_color, size,
             kwargs):
    import matplotlib.pyplot as plt
    mesh = ax.pcolormesh(X, Y, PDF, **kwargs)
    ax.set_xlabel(x)
    ax.set_ylabel(y)
    if title is not None:
        ax.set_title(title)
    if colorbar:
        plt.colorbar(mesh, ax=ax)
    if refval is not None:
        ax.scatter([refval[x]], [refval[y]], color=refval_color)
    if size is not None:
        ax.get_figure().set_size_inches(size)
    return ax


def plot_kde_1d(df, w, x, xmin=None, xmax=None, numx=50, ax=None, size=None,
                title=None, refval=None, refval_color="C1", kde=None, **kwargs):
    """Plot the 1-D KDE of column x (kde.py:134-171) -> the axis."""
    import matplotlib.pyplot as plt
    x_vals, pdf = kde_1d(df, w, x, xmin=xmin, xmax=xmax, numx=numx, kde=kde)
    if ax is None:
        _, ax = plt.subplots()
    return _draw_1d(ax, x_vals, pdf, x, xmin, xmax, title, refval, refval_color,
                    size, kwargs)


def plot_kde_1d_highlevel(history, x, m=0, t=None, xmin=None, xmax=None, numx=50,
                          ax=None, size=None, title=None, refval=None,
                          refval_color="C1", kde=None, **kwargs):
    """plot_kde_1d of generation t of model m (kde.py:77-131)."""
    df, w = DevicePopulation.of_history(history, m, t), None
    return plot_kde_1d(df, w, x, xmin, xmax, numx, ax, size, title, refval,
                       refval_color, kde, **kwargs)


def plot_kde_2d(df, w, x, y, xmin=None, xmax=None, ymin=None, ymax=None,
                numx=50, numy=50, ax=None, size=None, colorbar=True, title=None,
                refval=None, refval_color="C1", kde=None, **kwargs):
    """Plot the 2-D KDE of columns (x, y) (kde.py:323-365) -> the axis."""
    import matplotlib.pyplot as plt
    X, Y, PDF = kde_2d(df, w, x, y, xmin=xmin, xmax=xmax, ymin=ymin, ymax=ymax,
                       numx=numx, numy=numy, kde=kde)
    if ax is None:
        _, ax = plt.subplots()
    return _draw_2d(ax, X, Y, PDF, x, y, colorbar, title, refval, refval_color,
                    size, kwargs)


def plot_kde_2d_highlevel(history, x, y, m=0, t=None, xmin=None, xmax=None,
                          ymin=None, ymax=None, numx=50, numy=50, ax=None,
                          size=None, colorbar=True, title=None, refval=None,
                          refval_color="C1", kde=None, **kwargs):
    """plot_kde_2d of generation t of model m (kde.py:251-320)."""
    df, w = DevicePopulation.of_history(history, m, t), None
    return plot_kde_2d(df, w, x, y, xmin, xmax, ymin, ymax, numx, numy, ax, size,
                       colorbar, title, refval, refval_color, kde, **kwargs)


def plot_kde_matrix(df, w, limits=None, colorbar=True, height=2.5, numx=50,
                    numy=50, refval=None, refval_color="C1", kde=None,
                    arr_ax=None, scatter_max=10000):
    """KDE matrix of the 1-D and 2-D marginals (kde.py:421-515): the diagonal
    holds the 1-D KDEs, the lower triangle the 2-D ones, the upper triangle a
    scatter of the particles -> the [d, d] array of axes.

    scatter_max: a population of more particles is thinned to that many
    evenly spaced rows for the scatter (the reference draws every particle);
    None draws all."""
    import matplotlib.pyplot as plt
    pop = DevicePopulation(df, w)
    names = pop.names
    n_par = len(names)
    res = kde_matrix(pop, None, limits, numx, numy, kde)
    if arr_ax is None:
        fig, arr_ax = plt.subplots(nrows=n_par, ncols=n_par, sharex=False,
                                   sharey=False, squeeze=False,
                                   figsize=(height * n_par, height * n_par))
    else:
        fig = arr_ax[0, 0].get_figure()
    limits = {} if limits is None else limits
    default = (None, None)
    N = pop.X.shape[0]
    if scatter_max is not None and N > scatter_max:
        idx = np.round(np.linspace(0, N - 1, int(scatter_max))).astype(np.int64)
        pts = pop.X[gpu.as_dev(idx, dtype=gpu.I64, device=pop.X.device)].cpu().numpy()
    else:
        pts = pop.X.cpu().numpy()
    for i in range(n_par):
        yn = names[i]
        x_vals, pdf = res[(yn,)]
        lim = limits.get(yn, default)
        _draw_1d(arr_ax[i, i], x_vals, pdf, yn, lim[0], lim[1], None, refval,
                 refval_color, None, {})
        for j in range(i):
            xn = names[j]
            X, Y, PDF = res[(xn, yn)]
            _draw_2d(arr_ax[i, j], X, Y, PDF, xn, yn, colorbar, None, refval,
                     refval_color, None, {})
            ax = arr_ax[j, i]
            ax.scatter(pts[:, i], pts[:, j], color="k")
            if refval is not None:
                ax.scatter([refval[yn]], [refval[xn]], color=refval_color)
            ax.set_xlim(*limits.get(yn, default))
            ax.set_ylim(*limits.get(xn, default))
    format_plot_matrix(arr_ax, names)
    fig.tight_layout()
    return arr_ax


def plot_kde_matrix_highlevel(history, m=0, t=None, limits=None, colorbar=True,
                              height=2.5, numx=50, numy=50, refval=None,
                              refval_color="C1", kde=None, arr_ax=None,
                              scatter_max=10000):
    """plot_kde_matrix of generation t of model m (kde.py:368-418)."""
    df, w = DevicePopulation.of_history(history, m, t), None
    return plot_kde_matrix(df, w, limits, colorbar, height, numx, numy, refval,
                           refval_color, kde, arr_ax, scatter_max)
