"""GridSearchCV for transitions (pyabc/transition/model_selection.py:9-74).

The reference is a thin adapter over ``sklearn.model_selection.GridSearchCV``:
k contiguous folds (``KFold`` without shuffle), per fold and grid point one
``estimator.fit(X_train, w_train)`` and the score ``sum_i w_test,i log
pdf(x_test,i)`` (``Transition.score``, base.py:114-116), the grid point with
the best mean test score refitted to the whole population.

Device route.  The default grid varies only ``scaling`` of a
``MultivariateNormalTransition``, and scaling multiplies the covariance
(multivariatenormal.py:82): all grid points of a fold share one weighted
covariance and one whitening.  A fold is then one ``abc_weighted_moments`` +
``abc_mvn_fit`` at scaling 1 and one ``abc_mvn_logpdf_scaled`` call over the
held-out rows, which evaluates every scaling of the grid in one pass of the
cross-term GEMM.  The grid may also vary ``bandwidth_selector`` between the
two device rules; grid points that differ only in ``scaling`` are grouped.
Everything else (another estimator, a custom selector or scoring, a cv
object, other parameters) runs sklearn's own loop over ``Transition.fit`` /
``Transition.score``.
"""
import copy
import logging

import numpy as np
import pandas as pd
from sklearn.base import clone
from sklearn.model_selection import GridSearchCV as GridSearchCVSKL
from sklearn.model_selection import ParameterGrid

from .. import gpu
from .multivariatenormal import MultivariateNormalTransition, _bw_rule

logger = logging.getLogger("GridSearchCV")

DEVICE_PARAMS = ("scaling", "bandwidth_selector")
MAX_DEVICE_DIM = 59        # abc_mvn_logpdf_scaled: full rank r = d <= 59
MAX_SCALINGS = 64          # ... and at most 64 scalings per call


def kfold_bounds(n, k):
    """[start, stop) of the test block of each of ``KFold(k)``'s folds over n
    rows in order: the first n % k blocks have n // k + 1 rows."""
    sizes = np.full(k, n // k, dtype=np.int64)
    sizes[:n % k] += 1
    stops = np.cumsum(sizes)
    return [(int(b - s), int(b)) for s, b in zip(sizes, stops)]


def rank_scores(means):
    """sklearn's ``rank_test_score``: 1 is best, ties share the minimum rank,
    NaN means rank last (all NaN: all 1)."""
    from scipy.stats import rankdata
    means = np.asarray(means, dtype=np.float64)
    if np.isnan(means).all():
        return np.ones_like(means, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        filled = np.nan_to_num(means, nan=np.nanmin(means) - 1,
                               posinf=np.inf, neginf=-np.inf)
    return rankdata(-filled, method="min").astype(np.int32, copy=False)


def assemble_results(candidate_params, test_scores, train_scores=None):
    """``cv_results_`` (without the timing keys) and ``best_index_`` from
    score tables [n_candidates, n_splits], as BaseSearchCV._format_results
    does: unweighted mean, population std, min-rank of the mean test score,
    the first grid point of rank 1."""
    n = len(candidate_params)
    results = {}

    def store(name, table, rank=False):
        table = np.asarray(table, dtype=np.float64).reshape(n, -1)
        for f in range(table.shape[1]):
            results[f"split{f}_{name}"] = table[:, f]
        with np.errstate(invalid="ignore"):
            mean = np.average(table, axis=1)
            std = np.sqrt(np.average((table - mean[:, None]) ** 2, axis=1))
        results[f"mean_{name}"] = mean
        results[f"std_{name}"] = std
        if rank:
            results[f"rank_{name}"] = rank_scores(mean)

    names = sorted({k for p in candidate_params for k in p})
    for name in names:
        vals = np.ma.MaskedArray(np.empty(n, dtype=object), mask=True)
        for i, p in enumerate(candidate_params):
            if name in p:
                vals[i] = p[name]
        if not vals.mask.any() and all(
                isinstance(v, (int, float, np.integer, np.floating))
                and not isinstance(v, bool) for v in vals.data):
            vals = np.ma.MaskedArray(np.array(list(vals.data)), mask=False)
        results[f"param_{name}"] = vals
    results["params"] = list(candidate_params)
    store("test_score", test_scores, rank=True)
    if train_scores is not None:
        store("train_score", train_scores)
    best_index = int(results["rank_test_score"].argmin())
    return results, best_index


class GridSearchCV(GridSearchCVSKL):
    """Grid search over the parameters of a transition, e.g. the ``scaling``
    of :class:`MultivariateNormalTransition`, by cross-validated
    log-likelihood.  Parameters as for
    ``sklearn.model_selection.GridSearchCV``; defaults as in the reference:

    - estimator = MultivariateNormalTransition()
    - param_grid = {'scaling': np.linspace(0.05, 1.0, 5)}
    - cv = 5

    ``iid`` (removed from scikit-learn) is accepted and ignored.  After a
    search ``route_`` says which loop scored it: "device" (the fused kernel;
    ``cv_results_`` then has no timing keys) or "generic" (sklearn's).
    """

    def __init__(self, estimator=None, param_grid=None, scoring=None,
                 n_jobs=1, iid=True, refit=True, cv=5, verbose=0,
                 pre_dispatch='2*n_jobs', error_score='raise',
                 return_train_score=True):
        if estimator is None:
            estimator = MultivariateNormalTransition()
        if param_grid is None:
            param_grid = {'scaling': np.linspace(0.05, 1.0, 5)}
        self.best_estimator_ = None
        self.iid = iid
        super().__init__(
            estimator=estimator, param_grid=param_grid, scoring=scoring,
            n_jobs=n_jobs, pre_dispatch=pre_dispatch, cv=cv, refit=refit,
            verbose=verbose, error_score=error_score,
            return_train_score=return_train_score)

    # -- fit -----------------------------------------------------------------
    def fit(self, X, y=None, groups=None):
        """Fit the density estimator (perturber) to the sampled data: X the
        particles (DataFrame), y their weights."""
        if len(X) == 1 or len(X.columns) == 0:
            res = self.estimator.fit(X, y)
            self.best_estimator_ = self.estimator
            return res
        plan = self._device_plan(len(X), X.shape[1])
        if plan is None:
            return self._fit_generic(X, y, groups)
        gpu.require_device()
        Xd = gpu.as_dev(X.values)
        wd = gpu.as_dev(np.asarray(y, dtype=np.float64))
        self._device_search(Xd, wd, list(X.columns), plan)
        if self.refit:
            self.best_estimator_.fit(X, y)
        logger.info("Best params: %s", self.best_params_)
        return self

    def fit_device(self, Xd, wd, columns):
        """The same search on device tensors (the batched sampler's entry):
        Xd [N, d], wd [N] float64 (w normalised), columns = parameter names.
        No DataFrame round trip on the device route; the generic route copies
        the population to the host once."""
        N, d = Xd.shape
        columns = list(columns)
        if N == 1 or d == 0:
            res = self.estimator.fit_device(Xd, wd, columns)
            self.best_estimator_ = self.estimator
            return res
        plan = self._device_plan(N, d)
        if plan is None or not hasattr(self.estimator, "fit_device"):
            X = pd.DataFrame(Xd.cpu().numpy(), columns=columns)
            return self._fit_generic(X, wd.cpu().numpy(), None)
        self._device_search(Xd, wd, columns, plan)
        if self.refit:
            self.best_estimator_.fit_device(Xd, wd, columns)
        return self

    def _fit_generic(self, X, y, groups):
        """sklearn's loop, with the reference's reduction of an integer cv
        larger than the population."""
        self.route_ = "generic"
        extra = {} if groups is None else {"groups": groups}
        if isinstance(self.cv, (int, np.integer)) and self.cv > len(X):
            old_cv = self.cv
            self.cv = len(X)
            try:
                res = super().fit(X, y, **extra)
            finally:
                self.cv = old_cv
            logger.info("Reduced CV Gridsearch %s -> %s. Best params: %s",
                        old_cv, len(X), self.best_params_)
            return res
        res = super().fit(X, y, **extra)
        logger.info("Best params: %s", self.best_params_)
        return res

    # -- device route --------------------------------------------------------
    def _device_plan(self, N, d):
        """(candidate params, folds, groups) if the search can take the
        device route, else None.  groups: {bandwidth rule: [(candidate index,
        scaling)]}."""
        est = self.estimator
        if not isinstance(est, MultivariateNormalTransition):
            return None
        if self.scoring is not None or not (1 <= d <= MAX_DEVICE_DIM):
            return None
        if isinstance(self.cv, bool) or not isinstance(self.cv, (int, np.integer)):
            return None
        k = min(int(self.cv), N)
        if k < 2:
            return None
        folds = kfold_bounds(N, k)
        # a one-row train set is the reference's diag(|x|) covariance: the
        # estimator's own fit
        if N - max(b - a for a, b in folds) < 2:
            return None
        try:
            candidates = list(ParameterGrid(self.param_grid))
        except (TypeError, ValueError):
            return None                      # sklearn reports the bad grid
        if not candidates:
            return None
        groups = {}
        for i, params in enumerate(candidates):
            if any(name not in DEVICE_PARAMS for name in params):
                return None
            rule = _bw_rule(params.get("bandwidth_selector", est.bandwidth_selector))
            s = params.get("scaling", est.scaling)
            if rule is None or isinstance(s, bool) or \
                    not isinstance(s, (int, float, np.integer, np.floating)) or \
                    not (0 < float(s) < np.inf):
                return None
            groups.setdefault(rule, []).append((i, float(s)))
        return candidates, folds, groups

    def _device_search(self, Xd, wd, columns, plan):
        torch = gpu.torch
        candidates, folds, groups = plan
        self.route_ = "device"
        N, d = Xd.shape
        nc, k = len(candidates), len(folds)
        train = bool(self.return_train_score)
        # queue every fold's train set and its fits; read all stats at once
        sets, fits = [], {}
        for f, (a, b) in enumerate(folds):
            Xtr = torch.cat((Xd[:a], Xd[b:])).contiguous()
            wtr = torch.cat((wd[:a], wd[b:]))
            # TransitionMeta.wrap_fit: w /= w.sum() unless np.isclose(sum, 1)
            s = wtr.sum()
            close = (s - 1.0).abs() <= 1e-8 + 1e-5
            wtr = (wtr / torch.where(close, torch.ones_like(s), s)).contiguous()
            sets.append((Xtr, wtr))
            mom = gpu.weighted_moments_dev(Xtr, wtr)
            for rule in groups:
                fits[f, rule] = (mom, gpu.mvn_fit(mom, d, 1.0, rule))
        keys = list(fits)
        stats = torch.stack([fits[key][1][5] for key in keys]).cpu().numpy()
        test = np.empty((nc, k))
        trn = np.empty((nc, k)) if train else None
        pending = []
        for key, st in zip(keys, stats):
            f, rule = key
            a, b = folds[f]
            Xtr, wtr = sets[f]
            Xte, wte = Xd[a:b], wd[a:b]
            idx = [i for i, _ in groups[rule]]
            if st[7] == 0:
                raise ValueError("The input matrix must be symmetric positive "
                                 "semidefinite.")
            if int(st[0]) < d:
                # singular covariance: the estimator's own fit and its direct
                # kernel with the support mask, one grid point at a time
                for i in idx:
                    est = clone(self.estimator).set_params(**candidates[i])
                    est.fit_device(Xtr, wtr, columns)
                    sc = [(est.logpdf_device(Xte) * wte).sum()]
                    if train:
                        sc.append((est.logpdf_device(Xtr) * wtr).sum())
                    pending.append(([i], f, torch.stack(sc)[:, None]))
                continue
            mom, (_, _, _, U, _, _) = fits[key]
            mu = mom[2:2 + d]
            for c0 in range(0, len(idx), MAX_SCALINGS):
                part = groups[rule][c0:c0 + MAX_SCALINGS]
                sv = np.array([s for _, s in part])
                lc = -0.5 * (d * gpu.LOG_2PI + float(st[1]) + d * np.log(sv))
                sc = [gpu.mvn_logpdf_scaled(Xte, Xtr, wtr, mu, U, sv, lc, wt=wte)[1]]
                if train:
                    sc.append(gpu.mvn_logpdf_scaled(Xtr, Xtr, wtr, mu, U, sv, lc,
                                                    wt=wtr)[1])
                pending.append(([i for i, _ in part], f, torch.stack(sc)))
        # one read of every score
        flat = torch.cat([sc.reshape(-1) for _, _, sc in pending]).cpu().numpy()
        o = 0
        for idx, f, sc in pending:
            n = len(idx)
            test[idx, f] = flat[o:o + n]
            o += n
            if train:
                trn[idx, f] = flat[o:o + n]
                o += n
        self._store_results(candidates, test, trn, k)

    def _store_results(self, candidates, test, trn, n_splits):
        results, best = assemble_results(candidates, test, trn)
        self.cv_results_ = results
        self.n_splits_ = n_splits
        self.multimetric_ = False
        self.scorer_ = None
        self.best_index_ = best
        self.best_score_ = float(results["mean_test_score"][best])
        self.best_params_ = results["params"][best]
        if self.refit:
            self.best_estimator_ = clone(self.estimator).set_params(
                **clone(self.best_params_, safe=False))

    # -- the fitted transition (real methods: ABCSMC tests for them with
    #    hasattr before the first fit) ---------------------------------------
    def logpdf_device(self, xd, out=None, hint=None):
        kwargs = {} if out is None else {"out": out}
        return self.best_estimator_.logpdf_device(xd, hint=hint, **kwargs)

    def propose_device(self, *args, **kwargs):
        return self.best_estimator_.propose_device(*args, **kwargs)

    def proposal_arrays(self):
        return self.best_estimator_.proposal_arrays()

    def pdf(self, x):
        return self.best_estimator_.pdf(x)

    def rvs(self, size=None):
        return self.best_estimator_.rvs(size)

    def rvs_single(self):
        return self.best_estimator_.rvs_single()

    def __deepcopy__(self, memo):
        # as Transition.__deepcopy__: device tensors are immutable after the
        # fit and shared (the fitted estimator shares its own)
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for key, v in self.__dict__.items():
            new.__dict__[key] = v if key.startswith("_dev") else copy.deepcopy(v, memo)
        return new

    def __getattr__(self, item):
        if item == "best_estimator_":
            raise AttributeError(item)
        return getattr(self.best_estimator_, item)
