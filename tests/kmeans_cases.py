"""Inputs of the exact k-means tests (test_kmeans_ref_cpu.py on the host,
test_gpu_kmeans_exact.py on the device) and sklearn's fits of them, each made
once per process.  numpy and sklearn only."""
import functools

import numpy as np

# ---- case A: designed blobs ------------------------------------------------
# sizes straddle the 65 536-element block of the device passes
BLOB_SIZES = (65535, 65537, 1000, 131072 + 5, 7, 3)
BLOB_PLACEMENTS = ((0.0, 1.0, 1e-3), (1000.0, 0.5, 5e-4), (-3.0, 0.01, 1e-5))   # (base, sep, w)


@functools.lru_cache(maxsize=None)
def blobs(placement):
    """-> (x float32 shuffled, blob of origin per element, float64 mean of each blob's float32 values)."""
    base, sep, w = BLOB_PLACEMENTS[placement]
    rng = np.random.default_rng(100 + placement)
    origin = np.repeat(np.arange(len(BLOB_SIZES)), BLOB_SIZES)
    x = (base + sep * origin + w * rng.standard_normal(origin.size)).astype(np.float32)
    perm = rng.permutation(origin.size)
    x, origin = x[perm], origin[perm]
    means = np.array([x[origin == j].astype(np.float64).mean() for j in range(len(BLOB_SIZES))])
    x.setflags(write=False)
    origin.setflags(write=False)
    return x, origin, means


# ---- case B: Gaussians far from zero -----------------------------------------
GAUSS_OFFSETS = (0.0, 1.0, 10.0, 1000.0)
GAUSS_N = 2 * 65536 + 17
GAUSS_CAPPED = (0.0, 1.0)   # offsets at which few elements lie within a float32 ulp of a midpoint (test_kmeans_ref_cpu.py)


@functools.lru_cache(maxsize=None)
def gauss(off):
    x = (off + 0.02 * np.random.default_rng(7).standard_normal(GAUSS_N)).astype(np.float32)
    x.setflags(write=False)
    return x


# ---- case C: every k branch --------------------------------------------------
BRANCH_KS = (1, 2, 7, 8, 9, 16, 17, 32)
BRANCH_N = 65536 + 3


@functools.lru_cache(maxsize=None)
def uniform(n, tag=0):
    x = np.random.default_rng(1000 * tag + n).uniform(-1, 1, n).astype(np.float32)
    x.setflags(write=False)
    return x


_FITS = {}


def sklearn_fit(key, x, k):
    """KMeans(k, n_init=6) of x, fitted once per key -> (sorted centres float64, labels in that order, inertia_)."""
    if key not in _FITS:
        from sklearn.cluster import KMeans
        km = KMeans(n_clusters=k, n_init=6, random_state=0).fit(np.asarray(x).reshape(-1, 1))
        order = np.argsort(km.cluster_centers_[:, 0])
        inv = np.empty(k, np.int64)
        inv[order] = np.arange(k)
        _FITS[key] = (km.cluster_centers_[order, 0].astype(np.float64), inv[km.labels_], float(km.inertia_))
    return _FITS[key]


def inertia64(x, centres):
    """Inertia of the nearest-centre assignment, float64 on the host."""
    x = np.asarray(x, np.float64).reshape(-1)
    best = np.full(x.size, np.inf)
    for c in np.asarray(centres, np.float64).reshape(-1):
        best = np.minimum(best, (x - c) ** 2)
    return float(best.sum())
