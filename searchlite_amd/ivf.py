"""Centroids for GpuIndex.cluster_vector_field: a plain seeded Lloyd k-means in numpy on the host.  The index takes
whatever centroids the caller supplies; this is the helper for callers that have none and hold the vectors on the
host.  GpuIndex.train_vector_field (slg_index_train_vector_field) trains on the device instead, over the store the
index already holds, and needs neither numpy nor the vectors; its centroids can start from this helper's through
`init`."""
from __future__ import annotations

from typing import Optional

import numpy as np

COSINE, L2 = 0, 1


def _unit(x: np.ndarray) -> np.ndarray:
    n = np.linalg.norm(x, axis=1, keepdims=True)
    return x / np.where(n > 0, n, 1.0)


def _assign(x: np.ndarray, cent: np.ndarray, metric: int, block: int = 16384) -> np.ndarray:
    """The nearest centroid of every row (ties: the lowest id), block by block."""
    out = np.empty(len(x), np.int64)
    c2 = (cent * cent).sum(axis=1)
    for b in range(0, len(x), block):
        dots = x[b:b + block] @ cent.T
        # cosine over unit centroids: the greatest dot product; L2: the smallest |c|^2 - 2 x.c
        out[b:b + block] = np.argmax(dots if metric == COSINE else 2.0 * dots - c2, axis=1)
    return out


def train_centroids(values, n_lists: int, metric: int, iters: int = 8, seed: int = 0,
                    sample: Optional[int] = None) -> np.ndarray:
    """-> f32 [min(n_lists, rows), dim] centroids of `values` (f32 [rows, dim]).  metric 0: spherical k-means
    (rows and centroids normalised, centroids re-normalised after every step); 1: Euclidean.  The start is `seed`'s
    choice of distinct rows, `sample` rows (all when None) are trained on, and a cluster that empties keeps its
    previous centroid.  The same arguments give the same bytes."""
    x = np.ascontiguousarray(values, dtype=np.float32)
    assert x.ndim == 2 and len(x) > 0 and n_lists >= 1
    rng = np.random.default_rng(seed)
    if sample is not None and sample < len(x):
        x = x[np.sort(rng.choice(len(x), int(sample), replace=False))]
    if metric == COSINE:
        x = _unit(x)
    k = min(int(n_lists), len(x))
    cent = x[np.sort(rng.choice(len(x), k, replace=False))].copy()
    for _ in range(int(iters)):
        a = _assign(x, cent, metric)
        counts = np.bincount(a, minlength=k)
        live = counts > 0
        # the rows cluster by cluster (a stable sort: the sums add up in row order), one sum per live cluster
        starts = np.cumsum(counts) - counts
        sums = np.add.reduceat(x[np.argsort(a, kind="stable")], starts[live], axis=0, dtype=np.float64)
        new = cent.copy()
        new[live] = (sums / counts[live, None]).astype(np.float32)
        if metric == COSINE:
            norm = np.linalg.norm(new, axis=1)
            ok = live & (norm > 0)  # (a cluster whose mean is the zero vector keeps its centroid too)
            new[ok] = new[ok] / norm[ok, None]
            new[~ok] = cent[~ok]
        cent = new.astype(np.float32)
    return np.ascontiguousarray(cent, dtype=np.float32)
