"""The device 1-D k-means (k_bkm_* in csrc/lossy_kmeans.h, k_km_label in lossy_single.h) held to
its contract exactly: fed with the centres a fit returns, tests/kmeans_ref.py
(float64 numpy) says what every rank, count, unique value and the inertia of
that fit must be.  test_kmeans_ref_cpu.py shows on the host that the same
reference describes sklearn's answer.

Per tensor (check_fit): ranks equal for every element and the sentinel kept
outside the tensors, counts equal, centres non-decreasing, uniq equal, the
returned inertia within INERTIA_REL of the float64 one (+ 1e-12 n (hi - lo)^2
for fits whose inertia is zero), the float64-nearest centre for every element
but the at most MAX_EXCLUDED within a float32 ulp of a midpoint (these must
still sit in a cluster beside that midpoint), two runs bit-identical.  The
cap on the excluded holds for every input but B at off 10 and 1000, whose
float32 grid is so coarse that hundreds of elements share the values next to
a midpoint whatever the centres (test_kmeans_ref_cpu.py counts them).

Cases: A designed blobs whose partition is known, five seeds; B Gaussians
at offsets up to 1000; C every k branch of k_bkm_acc / k_bkm_label with
n = 65539 and n = k in one launch; D degenerate inputs and the tie on a
midpoint; E kmeans_fit and kmeans_label; F the label table at k = 7, 8;
G NaN and +-inf.

Returned inertia against float64, worst relative error measured on an MI355X
(INERTIA_MEASURED below); the assertion is min(1e-4, 4 x measured):
  A blobs 2.6e-8 (placement 0; 2.1e-16 at base 1000, 0 at base -3)
  B offset Gaussians 3.1e-8 (off 10; 5.4e-9, 6.7e-9, 1.5e-16 at off 0, 1, 1000)
  C k branches 9.5e-9 (k = 16), 0 for every n = k tensor
  D degenerate 0: every inertia there is exactly 0
  E kmeans_fit 5.2e-9 (k = 1), F label table 2.4e-8 (the 9-element tensor, k = 8)
Before k_bkm_acc summed about its pivots (sums of the raw values) the same
figures, on the same MI355X, were: A 1.3e-1 (placement 0); B 1.1e-4, 2.2e-2
and 2.1e+2 at off 1, 10 and 1000; C 5.1e-7 (k = 7) to 1.1e-5 (k = 32) and
1e-9 absolute on the n = k tensors, whose inertia is 0; E 9.9e-5 (k = 6);
F 1.7e-4; and a NaN went unreported.
Quality at k = 16 / 32 (test_quality_at_large_k): 1.00597 / 1.00165 x sklearn
at max_exact = 8 and the same at 64 (both converge inside 8 passes).
"""
import gzip

import numpy as np
import pytest
import torch

from tests import kmeans_cases as K
from tests.kmeans_ref import kmeans_ref, midpoints32, nearest_check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0
MAX_EXCLUDED = 4
# worst |returned - float64| / float64 of each case on an MI355X
INERTIA_MEASURED = {"A": 2.6e-8, "B": 3.1e-8, "C": 9.5e-9, "D": 0.0, "E": 5.2e-9, "F": 2.4e-8}
INERTIA_REL = {case: min(1e-4, 4 * worst) for case, worst in INERTIA_MEASURED.items()}


def _arena(xs, lead=1):
    """The tensors in one float32 arena, none at a 16-byte aligned offset."""
    offs, acc = [], lead
    for x in xs:
        if acc % 4 == 0:
            acc += 1
        offs.append(acc)
        acc += x.size + 2
    arena = torch.zeros(acc + 5, dtype=torch.float32, device=DEV)
    for x, o in zip(xs, offs):
        arena[o:o + x.size] = torch.from_numpy(np.array(x)).to(DEV)
    return arena, offs


def _fit(xs, k, **kw):
    """kmeans_batch of xs, twice: bit-identical; -> (offs, c, cnt, inertia, uniq, ranks arena on the host)."""
    from openfl_amd import lossy
    arena, offs = _arena(xs)
    outs = []
    for _ in range(2):
        ranks = torch.full_like(arena, SENTINEL)
        c, cnt, inertia, uniq = lossy.kmeans_batch(arena, offs, [x.size for x in xs], k, n_init=6, ranks_out=ranks,
                                                   **kw)
        outs.append((c, cnt, inertia, uniq, ranks.cpu().numpy()))
    a, b = outs
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a[3], b[3]))
    assert a[4].tobytes() == b[4].tobytes()
    inside = np.zeros(arena.numel(), bool)
    for x, o in zip(xs, offs):
        inside[o:o + x.size] = True
    assert np.all(a[4][~inside] == np.float32(SENTINEL))
    return (offs,) + a


def check_fit(x, c, cnt, inertia, uniq, ranks, value_f64, rel, cap=MAX_EXCLUDED, tag=""):
    """One tensor's results against the reference fed with its centres; -> the inertia's relative error."""
    assert np.all(np.isfinite(c)) and np.all(np.diff(c) >= 0), (tag, c)
    r = kmeans_ref(x, c, value_f64)
    np.testing.assert_array_equal(cnt, r.count, err_msg=tag)
    assert uniq.dtype == r.uniq.dtype and np.array_equal(uniq, r.uniq), (tag, uniq, r.uniq)
    assert ranks.dtype == np.float32
    np.testing.assert_array_equal(ranks, r.ranks, err_msg=tag)
    span = float(x.max()) - float(x.min())
    err = abs(inertia - r.inertia)
    relerr = err / r.inertia if r.inertia > 0 else 0.0
    print(f"kmeans-exact {tag}: inertia {inertia!r} float64 {r.inertia!r} rel {relerr:.3e}")
    assert err <= rel * r.inertia + 1e-12 * x.size * span * span, (tag, inertia, r.inertia, relerr)
    bad, excluded = nearest_check(x, c, r.cluster)
    assert bad == 0, (tag, bad)
    assert cap is None or excluded <= cap, (tag, excluded)
    return relerr


# ---- A: designed blobs -------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_blobs_partition_and_centres(seed):
    """Three placements of six blobs of 65535, 65537, 1000, 131077, 7 and 3
    elements in one batch: the fit finds the blobs (counts, the blob of origin
    of every element) and every centre is within 64 * 2^-24 * (hi - lo) of
    the float64 mean of its blob: the worst case of the 64 float additions a
    thread makes of values taken relative to a pivot inside [lo, hi]."""
    cases = [K.blobs(p) for p in range(len(K.BLOB_PLACEMENTS))]
    xs = [x for x, _, _ in cases]
    offs, c, cnt, inertia, uniq, ranks = _fit(xs, 6, seed=seed)
    for p, (x, origin, means) in enumerate(cases):
        tag = f"A placement {K.BLOB_PLACEMENTS[p]} seed {seed}"
        rk = ranks[offs[p]:offs[p] + x.size]
        check_fit(x, c[p], cnt[p], inertia[p], uniq[p], rk, False, INERTIA_REL["A"], tag=tag)
        np.testing.assert_array_equal(cnt[p], K.BLOB_SIZES, err_msg=tag)
        np.testing.assert_array_equal(rk, origin.astype(np.float32), err_msg=tag)
        bound = 64 * 2.0 ** -24 * (float(x.max()) - float(x.min()))
        worst = np.max(np.abs(c[p] - means))
        print(f"kmeans-exact {tag}: centre error {worst:.3e} bound {bound:.3e}")
        assert worst <= bound, (tag, worst, bound)


# ---- B: Gaussians far from zero ----------------------------------------------
@pytest.mark.parametrize("off", K.GAUSS_OFFSETS)
def test_offset_gaussians(off):
    """off + 0.02 N(0, 1), 2 * 65536 + 17 elements: the contract, and the
    project's quality bound (host inertia <= 1.01 x sklearn KMeans(6, n_init=6)).
    The exclusion cap applies where the float32 grid lets it (K.GAUSS_CAPPED)."""
    x = K.gauss(off)
    offs, c, cnt, inertia, uniq, ranks = _fit([x], 6, seed=3, value_f64=True)
    check_fit(x, c[0], cnt[0], inertia[0], uniq[0], ranks[offs[0]:offs[0] + x.size], True, INERTIA_REL["B"],
              cap=MAX_EXCLUDED if off in K.GAUSS_CAPPED else None, tag=f"B off {off}")
    ref = K.sklearn_fit(("gauss", off), x, 6)[2]
    ours = K.inertia64(x, c[0])
    print(f"kmeans-exact B off {off}: host inertia {ours!r} sklearn {ref!r} ratio {ours / ref:.5f}")
    assert ours <= 1.01 * ref, (off, ours, ref)


# ---- C: every k branch ---------------------------------------------------------
@pytest.mark.parametrize("value_f64", (False, True), ids=("f32", "f64"))
@pytest.mark.parametrize("k", K.BRANCH_KS)
def test_every_k_branch(k, value_f64):
    """k on both sides of the KM1 = 7 / 15 / 31 instantiations, uniform(-1, 1)
    with 65539 elements (two blocks) and with k elements in one launch."""
    xs = [K.uniform(K.BRANCH_N), K.uniform(k, tag=1), K.uniform(K.BRANCH_N, tag=2), K.uniform(k, tag=3)]
    offs, c, cnt, inertia, uniq, ranks = _fit(xs, k, seed=11, value_f64=value_f64)
    for t, x in enumerate(xs):
        check_fit(x, c[t], cnt[t], inertia[t], uniq[t], ranks[offs[t]:offs[t] + x.size], value_f64,
                  INERTIA_REL["C"], tag=f"C k {k} n {x.size} tensor {t} f64 {value_f64}")


@pytest.mark.parametrize("k", (16, 32))
def test_quality_at_large_k(k):
    """Host inertia <= 1.01 x sklearn KMeans(k, n_init=6) on uniform(-1, 1),
    n = 65539, at the default max_exact = 8 (and at 64, which changes nothing:
    the exact passes converge before the cap)."""
    from openfl_amd import lossy
    x = K.uniform(K.BRANCH_N)
    ref = K.sklearn_fit(("uniform", k), x, k)[2]
    xd = torch.from_numpy(np.array(x)).to(DEV)
    ratios = {}
    for max_exact in (8, 64):
        c, _, _, _ = lossy.kmeans_batch(xd, [0], [x.size], k, n_init=6, seed=11, max_exact=max_exact)
        ratios[max_exact] = K.inertia64(x, c[0]) / ref
    print(f"kmeans-exact quality k {k}: inertia / sklearn at max_exact 8: {ratios[8]:.5f}, at 64: {ratios[64]:.5f}")
    assert ratios[8] <= 1.01 and ratios[64] <= 1.01, ratios


# ---- D: degenerate inputs ------------------------------------------------------
def test_degenerate_inputs():
    """A constant tensor, 3 distinct values for 6 clusters, n = k = 6, and
    65536 equal values with one outlier (one occupied bin at each end of the
    histogram, four clusters left empty)."""
    rng = np.random.default_rng(5)
    heavy = np.full(65537, 0.125, np.float32)
    heavy[40_000] = 3.0
    xs = [np.full(1000, 0.25, np.float32), np.repeat(np.float32([1.0, 2.0, 3.0]), 400),
          rng.uniform(-1, 1, 6).astype(np.float32), heavy, np.full(70_001, -1000.5, np.float32)]
    for value_f64 in (False, True):
        offs, c, cnt, inertia, uniq, ranks = _fit(xs, 6, seed=2, value_f64=value_f64)
        for t, x in enumerate(xs):
            check_fit(x, c[t], cnt[t], inertia[t], uniq[t], ranks[offs[t]:offs[t] + x.size], value_f64,
                      INERTIA_REL["D"], tag=f"D tensor {t} f64 {value_f64}")
        assert uniq[0].tolist() == [0.25] and inertia[0] == 0.0
        assert uniq[1].tolist() == [1.0, 2.0, 3.0] and sorted(cnt[1][cnt[1] > 0]) == [400, 400, 400]
        assert np.array_equal(uniq[2].astype(np.float32), np.sort(xs[2])) and np.all(cnt[2] == 1)
        assert uniq[3].tolist() == [0.125, 3.0] and sorted(cnt[3][cnt[3] > 0]) == [1, 65536]
        assert uniq[4].tolist() == [-1000.5] and inertia[4] == 0.0


def test_value_on_a_midpoint_goes_to_the_lower_cluster():
    from openfl_amd import lossy
    x = K.gauss(1.0)[:10_000].copy()
    xd = torch.from_numpy(x).to(DEV)
    c, _, _ = lossy.kmeans_fit(xd, 6, n_init=6, seed=1)
    mid = midpoints32(c)
    assert np.all(np.diff(mid) > 0)
    x[5] = mid[2]
    x[6] = np.nextafter(mid[2], np.float32(np.inf))
    x[7] = np.nextafter(mid[2], np.float32(-np.inf))
    out = lossy.kmeans_label(torch.from_numpy(x).to(DEV), c, np.arange(6)).cpu().numpy()
    assert out[5] == 2.0 and out[6] == 3.0 and out[7] == 2.0
    np.testing.assert_array_equal(out, kmeans_ref(x, c, True).cluster.astype(np.float32))


# ---- E: kmeans_fit and kmeans_label --------------------------------------------
@pytest.mark.parametrize("k", (1, 6, 32))
def test_kmeans_fit_is_the_batch_of_one(k):
    """ofl_kmeans1d_fit returns bit for bit what ofl_kmeans1d_batch returns
    for [x] with value_f64, and it meets the contract."""
    from openfl_amd import lossy
    x = K.gauss(1.0) if k == 6 else K.uniform(K.BRANCH_N)
    xd = torch.from_numpy(np.array(x)).to(DEV)
    c, cnt, inertia = lossy.kmeans_fit(xd, k, n_init=6, seed=4)
    ranks = torch.full_like(xd, SENTINEL)
    cb, cntb, inb, uniq = lossy.kmeans_batch(xd, [0], [x.size], k, n_init=6, seed=4, value_f64=True, ranks_out=ranks)
    assert c.tobytes() == cb[0].tobytes() and cnt.tobytes() == cntb[0].tobytes()
    assert np.float64(inertia).tobytes() == inb[0].tobytes()
    check_fit(x, c, cnt, inertia, uniq[0], ranks.cpu().numpy(), True, INERTIA_REL["E"],
              tag=f"E fit k {k}")


@pytest.mark.parametrize("k", (1, 6, 32))
@pytest.mark.parametrize("n", (1, 4096, 4097, 70_001))
def test_kmeans_label_vs_numpy(n, k):
    """k_km_label: one block, the first size with two, and later trips of the
    grid-stride loop; ranks an arbitrary permutation of non-integers; x a
    view 3 elements into its allocation; values on and next to midpoints."""
    from openfl_amd import lossy
    rng = np.random.default_rng(100 * k + n)
    c = np.sort(rng.uniform(-1, 1, k))
    rank_of = (rng.permutation(k) + 0.25 + rng.uniform(0, 0.5, k)).astype(np.float32)
    x = rng.uniform(-1.1, 1.1, n).astype(np.float32)
    mid = midpoints32(c)
    if k > 1 and n >= 4096:
        x[10:10 + mid.size] = mid
        x[100:100 + mid.size] = np.nextafter(mid, np.float32(np.inf))
        x[-mid.size:] = np.nextafter(mid, np.float32(-np.inf))
    buf = torch.full((n + 8,), 9.0, dtype=torch.float32, device=DEV)
    xd = buf[3:3 + n]
    xd.copy_(torch.from_numpy(x))
    assert xd.is_contiguous() and xd.data_ptr() == buf.data_ptr() + 12
    out = lossy.kmeans_label(xd, c, rank_of).cpu().numpy()
    cl = np.searchsorted(mid, x, side="left")
    np.testing.assert_array_equal(out, rank_of[cl])


# ---- F: the label table at its limit -------------------------------------------
@pytest.mark.parametrize("k", (7, 8))
def test_label_table_at_k_7_and_8(k):
    """gzip_ranks(x, label=) is byte for byte gzip_ranks(ranks) with seven and
    with eight clusters (ofl_label_rec holds 8 ranks and 7 midpoints)."""
    from openfl_amd import lossy
    xs = [K.uniform(9, tag=4), K.uniform(K.BRANCH_N)]
    arena, offs = _arena(xs)
    ranks = torch.zeros_like(arena)
    tab = lossy.LabelTable(len(xs), DEV)
    c, cnt, inertia, uniq = lossy.kmeans_batch(arena, offs, [x.size for x in xs], k, n_init=6, seed=9,
                                               ranks_out=ranks, label_out=tab)
    rk = ranks.cpu().numpy()
    for t, x in enumerate(xs):
        check_fit(x, c[t], cnt[t], inertia[t], uniq[t], rk[offs[t]:offs[t] + x.size], False, INERTIA_REL["F"],
                  tag=f"F k {k} tensor {t}")
    assert uniq[1].size == k
    z_ref = lossy.gzip_ranks(ranks)
    z = lossy.gzip_ranks(arena, label=tab)
    assert z == z_ref
    assert gzip.decompress(z) == rk.tobytes()


# ---- G: non-finite input ---------------------------------------------------------
@pytest.mark.parametrize("what", ("nan", "+inf", "-inf"))
def test_non_finite_input_is_refused(what):
    """One NaN (which min / max drop), +inf or -inf in 70 001 elements: CodecError."""
    from openfl_amd import lossy
    from openfl_amd._lib import CodecError
    x = K.gauss(0.0)[:70_001].copy()
    x[66_000] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[what]
    xd = torch.from_numpy(x).to(DEV)
    with pytest.raises(CodecError, match="non-finite"):
        lossy.kmeans_batch(xd, [0], [x.size], 6, n_init=6, seed=0)
    with pytest.raises(CodecError, match="non-finite"):
        lossy.kmeans_fit(xd, 6, n_init=6, seed=0)
