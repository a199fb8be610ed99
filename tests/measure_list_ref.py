"""float64 numpy restatements of the measure-list distances
(pyabc/distance/distance.py:667-873) over matrices, shared by
test_measure_list_host.py and test_gpu_measure_list.py, and the fixture
tests/golden/measure_list.npz (make_golden_measure_list.py)."""
import os

import numpy as np

from conftest import GOLDEN

U = 2.0 ** -53


def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, "measure_list.npz")))


def keys(S):
    return [f"y{k}" for k in range(S)]


def as_dicts(data):
    ks = keys(np.asarray(data).shape[1])
    return [dict(zip(ks, row)) for row in np.asarray(data, dtype=np.float64)]


def sample_of(fx, tag):
    return fx[f"{tag}__sample"].astype(np.float64)


def zscore(X, x0, use):
    """mean over the used keys of |(x - x0) / x0| (no zero observation)."""
    X, x0 = np.asarray(X, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    d = np.zeros(X.shape[0])
    for k in use:
        d = d + np.abs((X[:, k] - x0[k]) / x0[k])
    return d / len(use)


def ranged(X, x0, norm, use):
    """sum over the used keys of |(x - x0) / normalization| (norm in ``use``
    order)."""
    X, x0 = np.asarray(X, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    d = np.zeros(X.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        for n, k in zip(norm, use):
            d = d + np.abs((X[:, k] - x0[k]) / n)
    return d


def whitened(X, x0, W):
    """|W (x - x0)|_2 per row and the dot-product bound's |W| |x - x0| norm."""
    X, x0, W = (np.asarray(a, dtype=np.float64) for a in (X, x0, W))
    with np.errstate(invalid="ignore", over="ignore"):
        dx = X - x0
        d = np.linalg.norm(dx @ W.T, axis=1)
        mag = np.linalg.norm(np.abs(dx) @ np.abs(W).T, axis=1)
    return d, mag


def embed(W, use, S):
    """W over the used keys embedded into [S x S] (zero rows and columns)."""
    out = np.zeros((S, S))
    out[np.ix_(use, use)] = W
    return out


def gram_longdouble(X):
    """Column means, the centred Gram matrix and the two sums of its error
    bound, all in np.longdouble."""
    Xl = np.asarray(X, dtype=np.longdouble)
    m = Xl.mean(axis=0)
    c = Xl - m
    G = c.T @ c
    a = np.abs(c)
    return m, G, a.T @ a, a.sum(axis=0)


def cond2_gram(sample, use=None):
    c = np.asarray(sample, dtype=np.float64)
    if use is not None:
        c = c[:, use]
    c = c - c.mean(axis=0)
    w = np.linalg.eigvalsh(c.T @ c)
    return float(w[-1] / w[0])
