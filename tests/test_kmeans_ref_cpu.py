"""The float64 reference of the k-means labelling contract (tests/kmeans_ref.py)
against sklearn, on the host: what test_gpu_kmeans_exact.py holds the device
kernels to is first shown to describe sklearn's own answer."""
import numpy as np
import pytest

from tests import kmeans_cases as K
from tests.kmeans_ref import kmeans_ref, midpoints32, nearest_check

MAX_EXCLUDED = 4   # the cap test_gpu_kmeans_exact.py puts on the elements nearest_check leaves out


@pytest.mark.parametrize("placement", range(len(K.BLOB_PLACEMENTS)))
def test_reference_restates_sklearn_on_blobs(placement):
    """sklearn KMeans(6, n_init=6) finds the designed blobs; the reference fed
    with its centres gives the blob sizes, sklearn's labels (in rank order) and
    sklearn's inertia to rel 1e-4."""
    x, origin, means = K.blobs(placement)
    c, labels, inertia = K.sklearn_fit(("blobs", placement), x, 6)
    np.testing.assert_array_equal(labels, origin)
    for value_f64 in (False, True):
        r = kmeans_ref(x, c, value_f64)
        np.testing.assert_array_equal(r.count, K.BLOB_SIZES)
        np.testing.assert_array_equal(r.cluster, labels)
        np.testing.assert_array_equal(r.rank, np.arange(6))
        np.testing.assert_array_equal(r.ranks, labels.astype(np.float32))
        assert r.uniq.dtype == (np.float64 if value_f64 else np.float32) and r.uniq.size == 6
        assert abs(r.inertia - inertia) <= 1e-4 * inertia, (r.inertia, inertia)
    bad, excluded = nearest_check(x, c)
    assert bad == 0 and excluded <= MAX_EXCLUDED


@pytest.mark.parametrize("off", K.GAUSS_OFFSETS)
def test_offset_gaussians_stay_under_the_exclusion_cap(off):
    """With sklearn's centres the offset Gaussians leave at most MAX_EXCLUDED
    elements within a float32 ulp of a midpoint, and the reference's labels
    are the float64-nearest centres everywhere else.  From off = 10 on the cap
    cannot hold for any centres: 131 089 values 0.02 wide lie on a float32 grid
    of 9.5e-7 (off 10) or 6.1e-5 (off 1000), so each of the two or three grid
    values within an ulp of a midpoint is taken by several (18 in all here)
    or by hundreds (1280) of elements.  K.GAUSS_CAPPED names the offsets the
    device test may hold to the cap."""
    x = K.gauss(off)
    c, labels, inertia = K.sklearn_fit(("gauss", off), x, 6)
    r = kmeans_ref(x, c, True)
    bad, excluded = nearest_check(x, c, r.cluster)
    assert bad == 0
    assert (excluded <= MAX_EXCLUDED) == (off in K.GAUSS_CAPPED), excluded


@pytest.mark.parametrize("k", (16, 32))
def test_uniform_stays_under_the_exclusion_cap(k):
    x = K.uniform(K.BRANCH_N)
    c, labels, inertia = K.sklearn_fit(("uniform", k), x, k)
    bad, excluded = nearest_check(x, c)
    assert bad == 0 and excluded <= MAX_EXCLUDED


def test_tie_and_duplicate_rules_by_hand():
    """Eight elements, centres [0, 1, 1, 4]: midpoints 0.5, 1, 2.5.  0.5 sits
    on a midpoint and goes to the lower cluster; everything in (0.5, 1] goes
    to cluster 1 and nothing to cluster 2 (the duplicate), which np.unique
    then drops; the two used centres of value 1 share a rank."""
    c = np.array([0.0, 1.0, 1.0, 4.0])
    x = np.array([-1.0, 0.5, 0.5000001, 1.0, 1.0000001, 2.5, 2.5000005, 9.0], np.float32)
    np.testing.assert_array_equal(midpoints32(c), np.float32([0.5, 1.0, 2.5]))
    r = kmeans_ref(x, c, False)
    np.testing.assert_array_equal(r.cluster, [0, 0, 1, 1, 2, 2, 3, 3])
    np.testing.assert_array_equal(r.count, [2, 2, 2, 2])
    np.testing.assert_array_equal(r.uniq, np.float32([0.0, 1.0, 4.0]))
    np.testing.assert_array_equal(r.rank, [0, 1, 1, 2])
    np.testing.assert_array_equal(r.ranks, np.float32([0, 0, 1, 1, 1, 1, 2, 2]))
    assert r.inertia == pytest.approx(1 + 0.25 + (0.5000001 - 1) ** 2 + 0 + 1e-14 + 2.25 + (4 - 2.5000005) ** 2 + 25,
                                      rel=1e-6)
    # with the duplicate left empty, np.unique sees the used centres only
    r = kmeans_ref(np.float32([0.0, 0.9, 5.0]), c, True)
    np.testing.assert_array_equal(r.count, [1, 1, 0, 1])
    np.testing.assert_array_equal(r.uniq, [0.0, 1.0, 4.0])
    assert r.uniq.dtype == np.float64
    # a float32 value decides the rank when float64 centres differ below float32
    c2 = np.array([1.0, 1.0 + 1e-12, 3.0])
    x2 = np.float32([1.0, 1.0000001, 3.0])
    np.testing.assert_array_equal(kmeans_ref(x2, c2, False).ranks, np.float32([0, 0, 1]))
    np.testing.assert_array_equal(kmeans_ref(x2, c2, True).ranks, np.float32([0, 1, 2]))
    # nearest_check: values, not indices; 0.5 and 2.5 are on float64 midpoints
    assert nearest_check(x, c) == (0, 2)
    assert nearest_check(x, c, np.array([0, 1, 1, 1, 2, 2, 3, 3]))[0] == 0     # still excluded
    assert nearest_check(x, c, np.array([1, 0, 1, 1, 2, 2, 3, 3]))[0] == 1     # -1 is nearest to 0
