"""GPU: the aggregation kernels of csrc/agg_kernels.hip at every collaborator
count they branch on, and on the second trip of their grid-stride loops.

  1. the register median's compare-exchange networks, C = 1..16, proven on the
     device by all 2^C columns of zeros and ones (a network that is right on
     those is right on every NaN-free input), through the 16-byte body and
     through the scalar path;
  2. designed columns (NaN, +-inf, float32 overflow, subnormals, +-0) for every
     C of the register path and for the LDS path's counts;
  3. the LDS median at even / odd counts up to 128, on random, ascending and
     descending columns, with each combination of outputs;
  4. the weighted average: NumPy's pairwise order for single elements up to
     2048 collaborators, on inputs shown to tell the summation orders apart,
     and the chained launches at the multiples of 16;
  5. the adaptive step and the geometric median at the templated counts the
     other tests leave out;
  6. sizes, taken from the device's CU count, at which k_median, k_median_lds,
     k_wavg_delta and k_adaptive run their loops more than once.

The references are NumPy itself (np.median, np.average) and the restatements
that the CPU tests show equal to the reference's recorded results.  Everything
is compared bit for bit, except the median (by value: tied zeros may differ in
sign) and the geometric median (1e-10 * max|x|, as in
tests/test_gpu_robust_aggregation.py)."""
import numpy as np
import pytest
import torch

from tests.test_adaptive_aggregation_cpu import F, Restated, assert_same_bits
from tests.test_gpu_adaptive_aggregation import CUSTOM, KINDS, _local, _plugin, _weights
from tests.test_robust_aggregation_cpu import (GM_RTOL, MEDIAN_LDS_C, MEDIAN_REGISTER_C, WAVG_POINT_C, WAVG_POINTS,
                                               assert_designed_reference, assert_wavg_points_discriminate,
                                               designed_stack, median_reference, restate_geometric_median,
                                               rounds_decided, wavg_point_case, zero_one_columns)
from tests import adaptive_golden as AG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 9.0      # fills the arenas around the views a kernel may write
JUNK = -7.0     # fills the views a kernel must overwrite


# ------------------------------------------------------------- arenas ---
def _arenas(rows, offset, dtype=torch.float32, pad=3):
    """The rows of a 2-D host array as views of one device tensor, each view
    `offset` elements into its own 16-byte aligned row, sentinels around it.
    -> (tensor, views)."""
    rows = np.atleast_2d(rows)
    n = rows.shape[1]
    width = -(-(offset + n + pad) // 4) * 4
    t = torch.full((rows.shape[0], width), SENT, dtype=dtype, device=DEV)
    t[:, offset:offset + n] = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
    views = [t[c, offset:offset + n] for c in range(rows.shape[0])]
    assert all(v.data_ptr() % 16 == (v.element_size() * offset) % 16 for v in views)
    return t, views


def _output(n, offset, dtype, pad=3):
    """-> (tensor, view): JUNK where the kernel must write, sentinels around."""
    t = torch.full((1, -(-(offset + n + pad) // 4) * 4), SENT, dtype=dtype, device=DEV)
    t[:, offset:offset + n] = JUNK
    return t, t[0, offset:offset + n]


def _untouched(t, offset, n):
    return bool((t[:, :offset] == SENT).all()) and bool((t[:, offset + n:] == SENT).all())


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _ptrs(views):
    return np.asarray([v.data_ptr() for v in views], np.uint64)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _median_delta(xs, base, n, med, delta):
    from openfl_amd import _lib
    ptrs = _ptrs(xs)
    _lib.check_agg(_lib.lib().ofl_median_delta(len(xs), ptrs.ctypes.data, _ptr(base), int(n), _ptr(med), _ptr(delta),
                                               _stream()))


def _wavg_delta(xs, w64, wsum, base, n, agg, delta64, delta32):
    from openfl_amd import _lib
    ptrs, w64 = _ptrs(xs), np.ascontiguousarray(w64, np.float64)
    return _lib.lib().ofl_wavg_delta(len(xs), ptrs.ctypes.data, w64.ctypes.data, float(wsum), _ptr(base), int(n),
                                     _ptr(agg), _ptr(delta64), _ptr(delta32), _stream())


def _same_f64(got, ref, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.float64 and got.shape == ref.shape, what
    if got.tobytes() != ref.tobytes():
        bad = np.flatnonzero(got.view(np.uint64) != ref.view(np.uint64))
        raise AssertionError(f"{what}: {bad.size} elements differ, first at {bad[:5]}: got "
                             f"{[float(v).hex() for v in got[bad[:3]]]}, expected "
                             f"{[float(v).hex() for v in ref[bad[:3]]]}")


def _same_median(got, ref, what, labels=None):
    """By value, NaN exactly where NumPy puts it (-0.0 == 0.0)."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == F and ref.dtype == F and got.shape == ref.shape, what
    bad = np.flatnonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
    if labels is not None and bad.size:
        what += ": " + ", ".join(f"{labels[k]} (got {got[k]!r}, expected {ref[k]!r})" for k in bad[:6])
    np.testing.assert_array_equal(got, ref, err_msg=what)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what


def _spread(rng, C, n):
    """Random collaborators, one magnitude out of 1e-3..1e2 each."""
    return np.stack([(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3)).astype(F) for _ in range(C)])


# ---------------------------- 1. register median: the 0/1 proof, device ---
@pytest.mark.parametrize("C", MEDIAN_REGISTER_C)
def test_register_median_zero_one_proof(C):
    """All 2^C columns of zeros and ones through mednet::median_of<C> as the
    device build compiles it: first through median() (aligned: med_quad from
    C = 2 on), then through ofl_median_delta on views offset by one element
    (every column through med_elem) with a base and both outputs.  The values
    are +0, 0.5 and 1, so the comparison is bit for bit."""
    from openfl_amd import aggregation
    stack = zero_one_columns(C)
    n = stack.shape[1]
    ref = np.median(stack, axis=0)
    assert ref.dtype == F
    assert_same_bits(aggregation.median(list(stack), DEV), ref, f"C={C} median()")

    base = np.random.default_rng(C).standard_normal(n).astype(F)
    tx, xs = _arenas(stack, 1)
    tb, (b,) = _arenas(base, 1)
    tm, med = _output(n, 1, torch.float32)
    td, delta = _output(n, 1, torch.float32)
    _median_delta(xs, b, n, med, delta)
    assert_same_bits(med.cpu().numpy(), ref, f"C={C} median_out, scalar path")
    assert_same_bits(delta.cpu().numpy(), ref - base, f"C={C} delta_out, scalar path")
    assert _untouched(tm, 1, n) and _untouched(td, 1, n)
    assert torch.equal(tx[:, 1:1 + n].cpu(), torch.from_numpy(stack))       # the inputs are left as they were


# -------------------------------- 2. designed columns, both median paths ---
@pytest.mark.parametrize("C", MEDIAN_REGISTER_C + MEDIAN_LDS_C)
def test_median_designed_columns_every_count(C):
    """designed_columns(C), forward and reversed (62 + 4 C columns: a 16-byte
    body and a tail of two), against np.median; NaN exactly where NumPy has it."""
    from openfl_amd import aggregation
    stack, labels = designed_stack(C)
    ref = median_reference(stack)
    assert_designed_reference(C, stack, ref)
    _same_median(aggregation.median(list(stack), DEV), ref, f"C={C}", labels)


# ---------------------------------------- 3. LDS median: counts, orders ---
@pytest.mark.parametrize("C", MEDIAN_LDS_C)
def test_lds_median_counts_and_orders(C):
    """k_median_lds with even and odd counts up to the limit, n = 64 * 3 + 5
    (three full blocks and a partial one), on random columns and on the same
    columns ascending (no shift in the insertion sort) and descending (the
    longest shift); median_out only, delta_out only, both with a base."""
    n = 64 * 3 + 5
    rng = np.random.default_rng(300 + C)
    random = _spread(rng, C, n)
    base = rng.standard_normal(n).astype(F)
    tb, (b,) = _arenas(base, 0)
    for order, stack in (("random", random), ("ascending", np.sort(random, axis=0)),
                         ("descending", np.sort(random, axis=0)[::-1])):
        stack = np.ascontiguousarray(stack)
        ref = np.median(stack, axis=0)
        _, xs = _arenas(stack, 0)
        what = f"C={C} {order}"
        tm, med = _output(n, 0, torch.float32)
        _median_delta(xs, None, n, med, None)
        _same_median(med, ref, what + " median_out only")
        td, delta = _output(n, 0, torch.float32)
        _median_delta(xs, None, n, None, delta)
        _same_median(delta, ref, what + " delta_out only")
        assert _untouched(tm, 0, n) and _untouched(td, 0, n), what
        tm, med = _output(n, 0, torch.float32)
        td, delta = _output(n, 0, torch.float32)
        _median_delta(xs, b, n, med, delta)
        _same_median(med, ref, what + " median_out with a base")
        assert_same_bits(delta.cpu().numpy(), ref - base, what + " delta_out with a base")
        assert _untouched(tm, 0, n) and _untouched(td, 0, n), what


# ------------------ 4. weighted average: pairwise order, chained launches ---
@pytest.mark.parametrize("with_base", [True, False])
@pytest.mark.parametrize("C", WAVG_POINT_C)
def test_wavg_points_pairwise_order(C, with_base):
    """ofl_wavg_delta_points on 256 single-element tensors in one call: NumPy's
    pairwise order at the 7/8 and 128/129 boundaries and through the recursive
    split (halves rounded down to a multiple of 8) up to 2048 collaborators.
    The inputs are first shown to tell that order from the in-order sum and
    from one unsplit block (tests/test_robust_aggregation_cpu.py)."""
    from openfl_amd import _lib
    case = wavg_point_case(C)
    assert_wavg_points_discriminate(C, case)
    n = WAVG_POINTS
    _, xs = _arenas(case["x"], 0)
    tb, (b,) = _arenas(case["base"], 0)
    ta, agg = _output(n, 0, torch.float64)
    t64, d64 = _output(n, 0, torch.float64)
    t32, d32 = _output(n, 0, torch.float32)
    L = _lib.lib()
    ws = torch.empty(int(L.ofl_wavg_points_workspace_bytes(C, n)), dtype=torch.uint8, device=DEV)
    ptrs, idx, w = _ptrs(xs), np.arange(n, dtype=np.int64), np.ascontiguousarray(case["w"], np.float64)
    _lib.check_agg(L.ofl_wavg_delta_points(C, ptrs.ctypes.data, w.ctypes.data, case["wsum"],
                                           _ptr(b) if with_base else None, n, idx.ctypes.data, _ptr(agg), _ptr(d64),
                                           _ptr(d32), ws.data_ptr(), ws.numel(), _stream()))
    what = f"C={C} base={with_base}"
    ref64 = case["delta64"] if with_base else case["avg"]
    _same_f64(agg, case["avg"], what + " agg_out")
    _same_f64(d64, ref64, what + " delta64_out")
    assert_same_bits(d32.cpu().numpy(), ref64.astype(F), what + " delta32_out")
    assert _untouched(ta, 0, n) and _untouched(t64, 0, n) and _untouched(t32, 0, n), what


def test_weighted_average_single_element_collaborator_limit():
    """The public entry with shapes (1,) and (): above 128 collaborators and
    at the limit of 2048 equal to np.average; 2049 are refused."""
    from openfl_amd import _lib
    from openfl_amd.aggregation import weighted_average
    rng = np.random.default_rng(77)
    for C in (129, 2048):
        for shape in ((1,), ()):
            xs = [np.asarray(rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 3)).astype(F) for _ in range(C)]
            w = list(rng.random(C) * 5)
            ref = np.average(xs, weights=w, axis=0)
            got = weighted_average(xs, w, DEV)
            assert got.dtype == np.float64 and got.shape == ref.shape
            assert got.tobytes() == ref.tobytes(), (C, shape, got, ref)
    for shape in ((1,), ()):
        xs = [np.ones(shape, F)] * 2049
        with pytest.raises(_lib.CodecError):
            weighted_average(xs, [1.0] * 2049, DEV)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("C", [15, 16, 17, 31, 32, 33, 48, 49])
def test_wavg_chained_launch_boundaries(C, offset):
    """ofl_wavg_delta with agg_out around the multiples of 16 collaborators
    (one, two, three and four launches chained through agg_out), on 16-byte
    aligned views (the vector body and its tail) and on views offset by one
    element (the scalar path); n = 5, 1027 (a body and a tail), 4099 (more
    than one block)."""
    from openfl_amd import _lib
    for n in (5, 1027, 4099):
        rng = np.random.default_rng(1000 * C + n)
        stack = _spread(rng, C, n)
        w = rng.random(C) * 5
        base = rng.standard_normal(n).astype(F)
        avg, wsum = np.average(stack, weights=w, axis=0, returned=True)
        d64 = avg - base.astype(np.float64)
        _, xs = _arenas(stack, offset)
        _, (b,) = _arenas(base, offset)
        ta, agg = _output(n, offset, torch.float64)
        t64, o64 = _output(n, offset, torch.float64)
        t32, o32 = _output(n, offset, torch.float32)
        _lib.check_agg(_wavg_delta(xs, w, wsum[0], b, n, agg, o64, o32))
        what = f"C={C} n={n} offset {offset}"
        _same_f64(agg, avg, what + " agg_out")
        _same_f64(o64, d64, what + " delta64_out")
        assert_same_bits(o32.cpu().numpy(), d64.astype(F), what + " delta32_out")
        assert _untouched(ta, offset, n) and _untouched(t64, offset, n) and _untouched(t32, offset, n), what


def test_wavg_chained_needs_agg_out():
    from openfl_amd import _lib
    n, C = 1027, 17
    stack = _spread(np.random.default_rng(1), C, n)
    _, xs = _arenas(stack, 0)
    t64, o64 = _output(n, 0, torch.float64)
    t32, o32 = _output(n, 0, torch.float32)
    assert _wavg_delta(xs, np.ones(C), float(C), None, n, None, o64, o32) == _lib.OFL_EINVAL
    assert b"agg_out" in _lib.lib().ofl_agg_last_error()
    torch.cuda.synchronize()
    assert bool((o64 == JUNK).all()) and bool((o32 == JUNK).all())                 # nothing was launched
    assert _wavg_delta(xs[:16], np.ones(16), 16.0, None, n, None, o64, o32) == _lib.OFL_OK
    _same_f64(o64, np.average(stack[:16], weights=np.ones(16), axis=0), "16 collaborators without agg_out")


# ------------- 5. adaptive step and geometric median: every templated C ---
@pytest.mark.parametrize("C", list(range(5, 16)))
def test_adaptive_step_remaining_unrolled_counts(C):
    """k_adaptive<C> for the counts test_plugin_shapes_and_collaborator_counts
    leaves out: one step of every kind with non-default hyper-parameters,
    n = 5 and 1027 (a body and a tail), against the restatement."""
    w = _weights(C)
    for n in (5, 1027):
        for kind in KINDS:
            rng = np.random.default_rng(2000 * C + 10 * n + KINDS.index(kind))
            p0 = (rng.standard_normal(n) * 0.1).astype(F)
            base = (rng.standard_normal(n) * 0.1).astype(F)
            xs = [(base + rng.standard_normal(n) * 0.02).astype(F) for _ in range(C)]
            plug = _plugin(kind, params={"t": p0.copy()}, **CUSTOM[kind])
            r = Restated(kind, p0, **CUSTOM[kind])
            got = plug(_local(xs, w), AG.db_records("t", 0, base), "t", 0, ("trained",))
            what = f"C={C} n={n} {kind}"
            assert_same_bits(got, r.step(xs, w, base), what + " p")
            state = plug.state("t")
            assert_same_bits(state["second_moment"], r.v, what + " v")
            if kind != "adagrad":
                assert_same_bits(state["first_moment"], r.m, what + " m")


def gm_case(C):
    """C collaborators of n = 4096 + 513 elements (two chunks), one of them
    scaled and shifted away from the rest so that the weights move."""
    rng = np.random.default_rng(600 + C)
    n = 4096 + 513
    xs = [(rng.standard_normal(n) * 0.01).astype(F) for _ in range(C)]
    xs[C // 2] = xs[C // 2] * F(25) + F(0.3)
    return xs, list(rng.random(C) + 0.1)


@pytest.mark.parametrize("C", list(range(1, 17)))
def test_geometric_median_every_count(C):
    """k_gm_dist<C> and k_gm_final<C> for every C against the float64
    restatement (shown equal to the reference on the fixture cases) within
    1e-10 * max|x|; the same number of rounds wherever the restatement's
    stopping ratio is a decade from 1 at every round (it is for all sixteen:
    four rounds each); the same bytes twice.  Largest error seen on an
    MI355X: 2.6e-17 (C = 3; bound 1.2e-10)."""
    from openfl_amd.aggregation import geometric_median
    xs, w = gm_case(C)
    ref, ref_rounds, objs, ratios = restate_geometric_median(xs, w)
    got, rounds = geometric_median(xs, w, device=DEV, return_iterations=True)
    tol = GM_RTOL * max(float(np.abs(x).max()) for x in xs)
    err = float(np.abs(got - ref).max())
    print(f"C={C}: max|got - restated| = {err:.3e}, bound {tol:.3e}, rounds {rounds} (restated {ref_rounds}), "
          f"ratios {ratios}")
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert err <= tol
    if C > 1:   # the weights moved: not the plain weighted average
        assert np.abs(ref - np.average(xs, weights=w, axis=0)).max() > 1e-4
    if rounds_decided(ratios):
        assert rounds == ref_rounds
    assert geometric_median(xs, w, device=DEV).tobytes() == got.tobytes()


# ------------------------------ 6. second trip of the grid-stride loops ---
@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def pool(cus):
    """One run of random float32 values shared by the large cases:
    collaborator c of a case is a window of it, 61 c elements in."""
    n = 2 * cus * 16 * 1024 + 7
    return np.random.default_rng(6).standard_normal(n + 61 * 17, dtype=F)


def _windows(pool, C, n, scale=1.0):
    return np.stack([pool[61 * c:61 * c + n] * F(scale * (1 + c % 3)) for c in range(C)])


@pytest.mark.parametrize("offset", [0, 1])
def test_median_second_loop_trip(cus, pool, offset):
    """k_median<3> on more elements than one trip of the capped grid covers
    (16 blocks per CU x 256 threads x 4 elements): the vector body runs at
    least three trips and leaves a scalar tail; offset by one element the
    same length goes through the scalar loop, eight trips."""
    C, n = 3, 2 * cus * 16 * 1024 + 7
    assert n > cus * 16 * 1024
    stack = _windows(pool, C, n)
    ref = np.median(stack, axis=0)
    _, xs = _arenas(stack, offset, pad=67)
    tm, med = _output(n, offset, torch.float32, pad=67)
    _median_delta(xs, None, n, med, None)
    _same_median(med, ref, f"n={n} offset {offset}")
    assert _untouched(tm, offset, n)


def test_lds_median_second_loop_trip(cus, pool):
    """k_median_lds beyond its grid cap (4 x 16 blocks per CU of 64 threads):
    one full trip, one more block and a partial one."""
    C, n = 17, cus * 16 * 4 * 64 + 64 + 5
    assert n > cus * 16 * 4 * 64
    stack = _windows(pool, C, n)
    ref = np.median(np.ascontiguousarray(stack.T), axis=1)      # np.median over the collaborators, row-contiguous
    _, xs = _arenas(stack, 0, pad=67)
    tm, med = _output(n, 0, torch.float32, pad=67)
    _median_delta(xs, None, n, med, None)
    _same_median(med, ref, f"n={n}")
    assert _untouched(tm, 0, n)


@pytest.mark.parametrize("C", [3, 17])
def test_wavg_second_loop_trip(cus, pool, C):
    """k_wavg_delta beyond one trip of the capped grid, one launch (C = 3)
    and two chained launches (C = 17), with a base."""
    from openfl_amd import _lib
    n = 2 * cus * 16 * 1024 + 7
    assert n > cus * 16 * 1024
    stack = _windows(pool, C, n)
    rng = np.random.default_rng(60 + C)
    w = rng.random(C) * 5
    base = pool[::-1][:n].copy()
    avg = np.empty(n)
    for a in range(0, n, 1 << 20):       # np.average by column blocks: the same sums, a bounded temporary
        avg[a:a + (1 << 20)], wsum = np.average(stack[:, a:a + (1 << 20)], weights=w, axis=0, returned=True)
    d64 = avg - base.astype(np.float64)
    _, xs = _arenas(stack, 0, pad=67)
    _, (b,) = _arenas(base, 0, pad=67)
    ta, agg = _output(n, 0, torch.float64, pad=67)
    t64, o64 = _output(n, 0, torch.float64, pad=67)
    t32, o32 = _output(n, 0, torch.float32, pad=67)
    _lib.check_agg(_wavg_delta(xs, w, wsum[0], b, n, agg, o64, o32))
    _same_f64(agg, avg, f"C={C} agg_out")
    _same_f64(o64, d64, f"C={C} delta64_out")
    assert_same_bits(o32.cpu().numpy(), d64.astype(F), f"C={C} delta32_out")
    assert _untouched(ta, 0, n) and _untouched(t64, 0, n) and _untouched(t32, 0, n)


def test_adaptive_second_loop_trip(cus, pool):
    """k_adaptive<3> (adam) beyond one trip of the capped grid: p, m, v,
    agg_out and delta_out after one step against the restatement."""
    from openfl_amd import aggregation as A
    C, n, kind = 3, 2 * cus * 16 * 1024 + 7, "adam"
    assert n > cus * 16 * 1024
    w = _weights(C)
    base = pool[:n] * F(0.1)
    xs = [base + pool[61 * (c + 1):61 * (c + 1) + n] * F(0.02) for c in range(C)]
    r = Restated(kind, pool[::-1][:n] * F(0.1), **CUSTOM[kind])
    r.m, r.v = np.abs(pool[7:7 + n]) * F(0.01), np.abs(pool[13:13 + n]) * F(0.01)    # a state that varies by element
    _, vx = _arenas(np.stack(xs), 0, pad=67)
    _, (b,) = _arenas(base, 0, pad=67)
    (tp, (p,)), (tm, (m,)), (tv, (v,)) = (_arenas(a, 0, pad=67) for a in (r.p, r.m, r.v))
    ta, agg = _output(n, 0, torch.float32, pad=67)
    td, delta = _output(n, 0, torch.float32, pad=67)
    A.adaptive_step(A.AdaptiveHyper(kind, **CUSTOM[kind]), 0, vx, np.asarray(w, F), b, n, p, m, v, agg_out=agg,
                    delta_out=delta, device=DEV)
    ref = r.step(xs, w, base)
    assert_same_bits(p.cpu().numpy(), ref, "p")
    assert_same_bits(m.cpu().numpy(), r.m, "m")
    assert_same_bits(v.cpu().numpy(), r.v, "v")
    assert_same_bits(agg.cpu().numpy(), ref, "agg_out")
    assert_same_bits(delta.cpu().numpy(), ref - base, "delta_out")
    for t in (tp, tm, tv, ta, td):
        assert _untouched(t, 0, n)
