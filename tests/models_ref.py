"""Numpy (float64) replay of the multi-model candidate rounds.

Test infrastructure, built from the oracle's Philox replay.  The semantics are
the reference's (pyabc/smc.py:610-662 _generate_valid_proposal, :754-811 the
prior / transition / weight functions, random_variables.py:455-538
ModelPerturbationKernel, population.py _normalize_weights); only the random
stream differs (Philox keyed by the global candidate index), so the device and
this replay agree draw for draw.
"""
import numpy as np

import oracle
from oracle.philox import philox4x32_10, uniform53
from oracle.sampler import (SLOT_PERTURB, SLOTS_PER_ATTEMPT, perturbation_normals,
                            prior_draws, prior_logpdf, simulate_linear_gaussian)

SLOT_MODEL = SLOTS_PER_ATTEMPT - 1      # abc_candidate.h


def model_draw(index, attempt, model_cdf, generation, seed):
    """Model of candidates `index` in attempt `attempt`:
    searchsorted(model_cdf, u total, side="right") with u from words 0, 1 of
    the attempt's last slot; a model of zero mass is never drawn."""
    cdf = np.asarray(model_cdf, dtype=np.float64)
    last = int(np.nonzero(np.diff(np.concatenate([[0.0], cdf])) > 0)[0][-1])
    r = philox4x32_10(index, attempt * SLOTS_PER_ATTEMPT + SLOT_MODEL, generation, seed)
    u = uniform53(r[:, 0], r[:, 1])
    m = np.searchsorted(cdf[:last + 1], u * cdf[last], side="right")
    return np.minimum(m, last)


def attempt_theta(mod, index, attempt, generation, seed):
    """One attempt of the single-model proposal (oracle.sampler.propose_mvn /
    propose_prior, one pass of their loops) for candidates `index` in model
    `mod` (dict: kinds, params and, for a transition, X, cdf, L): theta,
    ancestor (-1: prior draw), in-support flag."""
    kinds, params = mod["kinds"], np.asarray(mod["params"], dtype=np.float64)
    d = len(kinds)
    s0 = attempt * SLOTS_PER_ATTEMPT
    if mod.get("X") is None:
        th = np.empty((len(index), d))
        for k in range(d):
            th[:, k], _ = prior_draws(kinds[k], params[k], index, s0 + 32 + 512 * k,
                                      generation, seed)
        j = np.full(len(index), -1, dtype=np.int64)
    else:
        X, cdf = np.asarray(mod["X"]), np.asarray(mod["cdf"])
        r = philox4x32_10(index, s0, generation, seed)
        u = uniform53(r[:, 0], r[:, 1])
        j = np.minimum(np.searchsorted(cdf, u * cdf[-1], side="right"), len(cdf) - 1)
        n = perturbation_normals(index, s0 + SLOT_PERTURB, d, generation, seed, r)
        th = X[j] + n @ np.asarray(mod["L"]).T
    ok = prior_logpdf(th, kinds, params) > -np.inf
    return th, j, ok


def propose(models, model_cdf, seed, generation, idx0, B, max_attempts=1000):
    """abc_models_propose replayed.  Every attempt draws the model anew and
    then theta in it (the reference restarts the whole attempt when theta
    leaves the support, smc.py:654-656).  Returns model [B], theta [B, d_max]
    (NaN past the model's d), ancestor, attempts (max_attempts + 1: gave up,
    model and theta of the last attempt) and the number of candidates whose
    model changed between two attempts."""
    dmax = max(len(m["kinds"]) for m in models)
    idx = np.arange(B, dtype=np.uint64) + np.uint64(idx0)
    model = np.zeros(B, dtype=np.int64)
    theta = np.full((B, dmax), np.nan)
    anc = np.full(B, -1, dtype=np.int64)
    att = np.full(B, max_attempts + 1, dtype=np.int64)
    changed = np.zeros(B, dtype=bool)
    todo = np.ones(B, dtype=bool)
    for a in range(max_attempts):
        pos = np.nonzero(todo)[0]
        if len(pos) == 0:
            break
        m_new = model_draw(idx[pos], a, model_cdf, generation, seed)
        if a > 0:
            changed[pos] |= m_new != model[pos]
        model[pos] = m_new
        for m in np.unique(m_new):
            sel = pos[m_new == m]
            th, j, ok = attempt_theta(models[m], idx[sel], a, generation, seed)
            theta[sel] = np.nan
            theta[sel, :th.shape[1]] = th
            anc[sel] = j
            att[sel[ok]] = a + 1
            todo[sel[ok]] = False
    return model, theta, anc, att, int(changed.sum())


def simulate(theta, model, src, a, sigma, seed, generation, idx0):
    """abc_models_simulate_linear_gaussian replayed: src, a, sigma [M, S]."""
    theta, model = np.asarray(theta), np.asarray(model)
    x = np.empty((len(theta), np.asarray(src).shape[1]))
    for m in np.unique(model):
        sel = model == m
        # the noise is keyed by the candidate's own index: simulate all rows
        # with model m's table and keep m's
        th = np.where(np.isnan(theta), 0.0, theta)
        x[sel] = simulate_linear_gaussian(th, src[m], a[m], sigma[m], seed, generation,
                                          idx0)[sel]
    return x


def partition(model, M):
    """(perm, counts): positions grouped by model, increasing within one."""
    model = np.asarray(model)
    return np.argsort(model, kind="stable"), np.bincount(model, minlength=M)


def kernel_matrix(M, stay):
    """K[n, m] = ModelPerturbationKernel(M, stay).pmf(n, m)
    (random_variables.py:455-538)."""
    if M == 1:
        return np.ones((1, 1))
    stay = 1.0 / M if stay is None else stay
    K = np.full((M, M), (1.0 - stay) / (M - 1))
    K[np.arange(M), np.arange(M)] = stay
    return K


def model_masses(p_prev, K, prior_pmf):
    """(q~ [M], model_factor [M]) from the previous generation's model
    probabilities p_prev ({m: p}, alive models only), the perturbation
    kernel's pmf matrix K[n, m] and the model prior's pmf.  model_factor(m) =
    sum_{m_prev} p_{m_prev} K(m | m_prev) (smc.py:792-795); q~ is the same
    sum, 0 for a dead target or one of prior mass 0 (smc.py:641-656)."""
    M = len(prior_pmf)
    mf = np.zeros(M)
    for m in range(M):
        mf[m] = sum(p * K[m, mp] for mp, p in p_prev.items())
    alive = np.array([m in p_prev and p_prev[m] > 0 and prior_pmf[m] > 0
                      for m in range(M)])
    return np.where(alive, mf, 0.0), mf


def weights(model, theta, models, mf, prior_pmf, covs):
    """w = pi(m) prior_m(theta) / (model_factor(m) T_m(theta)) per row
    (smc.py:754-811), T_m the model's KDE (oracle.mvn_logpdf) over its
    population (X, w) with covariance covs[m]."""
    w = np.empty(len(model))
    for m in np.unique(model):
        sel = model == m
        mod = models[m]
        d = len(mod["kinds"])
        th = theta[sel, :d]
        lp = prior_logpdf(th, mod["kinds"], mod["params"])
        lt = oracle.mvn_logpdf(th, np.asarray(mod["X"]), np.asarray(mod["w"]), covs[m])
        w[sel] = prior_pmf[m] * np.exp(lp - lt) / mf[m]
    return w


def normalize(model, w):
    """Population._normalize_weights (population.py:123-145): ({m: p_m},
    weights normalised within each model)."""
    model, w = np.asarray(model), np.asarray(w, dtype=np.float64)
    tot = {int(m): w[model == m].sum() for m in np.unique(model)}
    s = sum(tot.values())
    out = w.copy()
    for m, t in tot.items():
        out[model == m] /= t
    return {m: t / s for m, t in tot.items()}, out
