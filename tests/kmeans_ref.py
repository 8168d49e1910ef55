"""Plain float64 numpy restatement of the device 1-D k-means' labelling
contract (ofl_kmeans1d_batch / ofl_kmeans1d_label, include/ofl_codec.h), for
the tests: given the data and the sorted centres a fit returned, everything
else the fit returns follows.  No torch, no project imports.

  mid32[j]   = float32((c[j] + c[j+1]) / 2), sum and halving in float64
  cluster(v) = #{j : mid32[j] < v}: a value on a midpoint goes to the lower
               cluster
  count[j]   = #{i : cluster(x[i]) == j}
  value[j]   = c[j], or float32(c[j]) unless value_f64
  uniq       = np.unique(value[count > 0])
  rank[j]    = index of value[j] in uniq
  ranks[i]   = float32(rank[cluster(x[i])])
  inertia    = sum (x[i] - c[cluster(x[i])])^2 in float64
"""
from types import SimpleNamespace

import numpy as np


def midpoints32(c):
    c = np.asarray(c, np.float64)
    return ((c[:-1] + c[1:]) / 2).astype(np.float32)


def clusters(x, c):
    """cluster(v) for every element: mid32 is non-decreasing (float32 rounding
    is monotone), so the count of midpoints below v is a left bisection."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    return np.searchsorted(midpoints32(c), x.reshape(-1), side="left").astype(np.int64)


def kmeans_ref(x, c, value_f64):
    x = np.asarray(x)
    assert x.dtype == np.float32
    x = x.reshape(-1)
    c = np.asarray(c, np.float64).reshape(-1)
    k = c.size
    assert np.all(np.diff(c) >= 0), "centres must be sorted"
    cl = clusters(x, c)
    count = np.bincount(cl, minlength=k).astype(np.int64)
    value = c.copy() if value_f64 else c.astype(np.float32)
    uniq = np.unique(value[count > 0])
    rank = np.searchsorted(uniq, value)          # (clusters left empty: never looked up)
    ranks = rank[cl].astype(np.float32)
    inertia = float(np.sum((x.astype(np.float64) - c[cl]) ** 2))
    return SimpleNamespace(mid32=midpoints32(c), cluster=cl, count=count, value=value, uniq=uniq, rank=rank,
                           ranks=ranks, inertia=inertia)


def nearest_check(x, c, cluster=None):
    """The check that knows nothing of midpoints: the centre of each
    element's cluster must have the VALUE of the centre nearest to it in
    float64 (values, not indices: duplicate centres occur).  Elements within
    one float32 ulp of a float64 midpoint of two distinct centres are left
    out, where the float32 midpoint may legitimately fall on either side:
    those must still sit in one of the two clusters that meet there.
    -> (number of elements that disagree, number left out)."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    x64 = x.reshape(-1).astype(np.float64)
    c = np.asarray(c, np.float64).reshape(-1)
    cl = clusters(x, c) if cluster is None else np.asarray(cluster)
    best = np.full(x64.size, np.inf)
    near = np.zeros(x64.size, np.float64)
    for j in range(c.size):                      # (k passes over n, not an n x k matrix)
        d = np.abs(x64 - c[j])
        take = d < best
        best = np.where(take, d, best)
        near = np.where(take, c[j], near)
    skip = np.zeros(x64.size, bool)
    beside = np.zeros(x64.size, bool)
    u = np.unique(c)                             # (no boundary between two equal centres)
    for lo, hi in zip(u[:-1], u[1:]):
        m = (lo + hi) / 2
        at = np.abs(x64 - m) <= np.spacing(np.abs(np.float32(m))).astype(np.float64)
        skip |= at
        beside |= at & ((c[cl] == lo) | (c[cl] == hi))
    bad = np.where(skip, ~beside, c[cl] != near)
    return int(np.sum(bad)), int(np.sum(skip))
