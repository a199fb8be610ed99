"""Discrete random-walk transition for parameters on the integer grid
(pyabc/transition/randomwalk.py:9-83).

Each coordinate of a proposal is its ancestor's plus the sum of ``n_steps``
independent steps in {-1, 0, +1} with probabilities (p_l, p_c, p_r).  It is
the transition to pair with discrete priors (poisson, binom, ...).

The density is the mixture over the population of the product over
coordinates of the one-coordinate walk law P(s), s = x_k - X_jk.  P is a
table over s in [-n_steps, n_steps] (the trinomial sum of
randomwalk.py:99-118, formed once per parameter set), so a density is one
gather + product + weighted sum instead of one multinomial pmf per
(candidate, particle, coordinate, step count).

Two forms.  After a host ``fit`` (a DataFrame population) ``pdf`` and ``rvs``
are numpy code and need no GPU.  After ``fit_device`` (the batched sampler's
device-resident population, with a grid prior, random_variables.py) they run
the kernels of abc_walk.hip: the population packed to int32 (abc_walk_pack),
the density as an N_candidates x N_population pair loop of integer range
tests (abc_walk_logpmf), proposals drawn in one step per coordinate from the
net-displacement law by inverse CDF (abc_walk_propose: the law of the
reference's ``n_steps`` single steps, one uniform instead of ``n_steps``).
``logpdf_device`` / ``propose_device`` after a host fit upload the population
first.  The kernels take ``d <= 32`` and ``n_steps <= 512``; beyond that the
transition stays on the host path.
"""
from math import comb
from typing import Union

import numpy as np
import pandas as pd

from .base import DiscreteTransition


def walk_step_law(n_steps: int, p_l: float, p_r: float, p_c: float) -> np.ndarray:
    """P(net displacement = s) for s = -n .. n after n steps, as an array of
    2n + 1 entries (index s + n).  n_r right steps and n_l = n_r - s left steps
    leave n_c = n - n_r - n_l in place: multinomial(n; n_l, n_r, n_c)."""
    n = int(n_steps)
    law = np.zeros(2 * n + 1)
    for s in range(-n, n + 1):
        total = 0.0
        for n_r in range(max(s, 0), n + 1):
            n_l = n_r - s
            n_c = n - n_r - n_l
            if n_l < 0 or n_c < 0:
                continue
            total += (comb(n, n_r) * comb(n - n_r, n_l)
                      * p_r ** n_r * p_l ** n_l * p_c ** n_c)
        law[s + n] = total
    return law


class DiscreteRandomWalkTransition(DiscreteTransition):
    """Random walk of ``n_steps`` steps per coordinate from a weighted draw of
    the population (randomwalk.py:9-83).  Like the reference, it does not
    adapt to the population and is not a proper importance distribution
    (its support does not cover the prior's)."""

    def __init__(self, n_steps: int = 1, p_l: float = 1. / 3,
                 p_r: float = 1. / 3, p_c: float = 1. / 3):
        self.n_steps = n_steps
        self.p_l = p_l
        self.p_r = p_r
        self.p_c = p_c

    # limits of the kernels (include/abcgpu.h ABC_WALK_MAX_D / _MAX_STEPS)
    MAX_DEVICE_DIM = 32
    MAX_DEVICE_STEPS = 512

    def fit(self, X: pd.DataFrame, w: np.ndarray):
        # nothing to fit: TransitionMeta keeps X and the normalised w.  A
        # host fit is the numpy form: a device population of an earlier
        # fit_device is dropped
        self._drop_device()

    # -- device form ---------------------------------------------------------
    def _drop_device(self):
        for key in [k for k in self.__dict__ if k.startswith("_dev")]:
            del self.__dict__[key]

    def device_why_not(self, d):
        """Why the kernels cannot take this walk over d parameters ("" when
        they can)."""
        if not 1 <= int(self.n_steps) <= self.MAX_DEVICE_STEPS:
            return (f"DiscreteRandomWalkTransition n_steps = {self.n_steps} "
                    f"outside 1 .. {self.MAX_DEVICE_STEPS}")
        if not 1 <= d <= self.MAX_DEVICE_DIM:
            return (f"DiscreteRandomWalkTransition over {d} parameters "
                    f"(1 .. {self.MAX_DEVICE_DIM})")
        return ""

    def fit_device(self, Xd, wd, columns):
        """Device-resident fit used by the batched sampler: Xd [N, d], wd [N]
        float64 tensors (w normalised), columns = sorted parameter names.
        Raises the reference's ValueError (randomwalk.py:55-59) for a
        population that is not integer-valued (or beyond +-2^30).  A walk
        outside the kernels' limits keeps the host form."""
        from .exceptions import NotEnoughParticles
        from .multivariatenormal import _LazyArray, _LazyFrame
        if Xd.shape[0] == 0:
            raise NotEnoughParticles("Fitting not possible.")
        self.no_parameters = len(columns) == 0
        self.X = _LazyFrame(Xd, list(columns))
        self.w = _LazyArray(wd)
        self._drop_device()
        if self.no_parameters or self.device_why_not(Xd.shape[1]):
            return
        self._upload(Xd, wd)

    def _upload(self, Xd, wd):
        from .. import gpu
        Xi, bad = gpu.walk_pack(Xd)
        if int(bad.item()):          # one read per fit
            raise ValueError("Transition can only handle integer values, not "
                             f"fulfilled by {int(bad.item())} entries of the "
                             "population (or beyond +-2^30).")
        self._dev_X, self._dev_w, self._dev_Xi = Xd, wd, Xi
        self._dev_cdf = gpu.inclusive_scan(wd)
        self._dev_guide = gpu.cdf_guide(self._dev_cdf)
        self._seed = int(np.random.randint(0, 2 ** 62))
        self._counter = 0

    def _ensure_device(self):
        """The device form of the fitted population (uploaded on first use
        after a host fit)."""
        from .. import gpu
        if getattr(self, "_dev_X", None) is None:
            if self.X is None:
                raise ValueError("DiscreteRandomWalkTransition is not fitted")
            d = len(self.X.columns)
            why = self.device_why_not(d)
            if why:
                raise ValueError(why + ": no device form")
            gpu.require_device()
            self._upload(gpu.as_dev(np.asarray(self.X.values, dtype=np.float64)),
                         gpu.as_dev(np.asarray(self.w, dtype=np.float64)))
        key = (self.n_steps, self.p_l, self.p_r, self.p_c)
        if getattr(self, "_dev_law_key", None) != key:
            law = self._law()
            dev = self._dev_X.device
            self._dev_law = gpu.as_dev(law, device=dev)
            # the scan the proposals search: numpy's, so a replay on the
            # host holds the same bits
            self._dev_law_cum = gpu.as_dev(np.cumsum(law), device=dev)
            self._dev_law_last = int(np.nonzero(law > 0)[0][-1])
            self._dev_law_key = key

    def logpdf_device(self, xd, out=None, hint=None):
        """log mass at device points xd [M, d] (columns in fit order); -inf
        where the mass is 0, NaN for a row that is not integer-valued.
        hint: accepted for the interface of the continuous transitions."""
        from .. import gpu
        self._ensure_device()
        return gpu.walk_logpmf(xd, self._dev_Xi, self._dev_w, self._dev_law,
                               self.n_steps, out=out)

    def propose_device(self, B, grid_prior=None, seed=None, generation=0,
                       idx0=None, max_attempts=1):
        """Batched rvs: (theta [B, d], prior log mass, ancestor, attempts),
        re-drawn while the grid prior's mass is 0 (grid_prior: a
        gpu.GridPrior; None: plain rvs)."""
        from .. import gpu
        self._ensure_device()
        if idx0 is None:
            idx0 = self._counter
            self._counter += B
        return gpu.walk_propose(self._dev_Xi, self._dev_cdf, self._dev_guide,
                                self._dev_law_cum, self.n_steps, self._dev_law_last,
                                self._seed if seed is None else seed, generation,
                                idx0, B, max_attempts, grid_prior)

    def _law(self):
        key = (self.n_steps, self.p_l, self.p_r, self.p_c)
        if getattr(self, "_law_key", None) != key:
            self._law_table = walk_step_law(*key)
            self._law_key = key
        return self._law_table

    def _walk(self, size):
        """[size, dim] net displacements: n_steps steps per coordinate."""
        dim = len(self.X.columns)
        steps = np.random.choice([-1, 0, 1], p=[self.p_l, self.p_c, self.p_r],
                                 size=(self.n_steps, size, dim))
        return steps.sum(axis=0).astype(float)

    def rvs_single(self) -> pd.Series:
        if getattr(self, "_dev_X", None) is not None:
            theta = self.propose_device(1)[0].cpu().numpy()
            return pd.Series(theta[0], index=self.X.columns)
        start = self.X.sample(weights=self.w).iloc[0]
        return start + self._walk(1)[0]

    def rvs(self, size=None):
        if size is None:
            return self.rvs_single()
        if getattr(self, "_dev_X", None) is not None:
            theta = self.propose_device(size)[0].cpu().numpy()
            return pd.DataFrame(theta, columns=self.X.columns)
        idx = np.random.choice(len(self.X), size=size, p=np.asarray(self.w, float))
        vals = self.X.values[idx] + self._walk(size)
        return pd.DataFrame(vals, columns=self.X.columns)

    def pdf(self, x: Union[pd.Series, pd.DataFrame]) -> Union[float, np.ndarray]:
        """Probability mass at x; raises ValueError for non-integer x
        (randomwalk.py:55-70)."""
        if not np.all(np.isclose(x, x.astype(int))):
            raise ValueError(f"Transition can only handle integer values, not "
                             f"fulfilled by x={x}.")
        x = np.asarray(x[self.X.columns], dtype=float)
        single = x.ndim == 1
        xs = np.atleast_2d(x)
        if getattr(self, "_dev_X", None) is not None:
            from .. import gpu
            xd = gpu.as_dev(np.rint(xs), device=self._dev_X.device)
            out = gpu.torch.exp(self.logpdf_device(xd)).cpu().numpy()
            return float(out[0]) if single else out
        law = self._law()
        n = self.n_steps
        X = self.X.values.astype(float)
        w = np.asarray(self.w, dtype=float)
        out = np.empty(xs.shape[0])
        for i, row in enumerate(xs):
            s = np.rint(row[None, :] - X).astype(np.int64)          # [N, dim]
            inside = np.abs(s) <= n
            p = np.where(inside, law[np.clip(s + n, 0, 2 * n)], 0.0).prod(axis=1)
            out[i] = float(p @ w)
        return out[0] if single else out
