"""The label records on the device against numpy, on the designed rules and
layouts of tests/label_cases.py (checked on the host by test_label_cases_cpu.py):
k_label_apply through lossy.label_apply, the value records of k_bkm_tab through
lossy.kmeans_batch(value_out=), lossy.ternary_label_table, and the TLZ
encoder's lab_rank / lab_fill / lab_one through lossy.gzip_ranks(x, label=).

The reference is numpy alone: the cluster of a value is the number of the
record's midpoints below it, a NaN takes cluster 0, a value on a midpoint the
lower cluster; the backward is the literal loop of kc_pipeline.py:79-83.
Nothing the device computed enters a reference.  Everything is compared bit for
bit as uint32; NaN results (an infinite value on an opposite infinite base) by
position, since x86 and the GPU differ in the default NaN's sign.  No tolerance.

The sibling tests (test_label_apply_* in test_gpu_lossy_round_end.py,
test_gzip_label_fused_matches_rank_array in test_gpu_lossy.py,
test_label_table_at_k_7_and_8 in test_gpu_kmeans_exact.py) stay: they pin the
kernels to each other on fitted random data.

On an MI355X: the module 4 s, the slowest test 0.2 s.
"""
import functools
import gzip
import math

import numpy as np
import pytest
import torch

from tests import label_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
ROTS = range(len(C.VALUE_SETS))


def _view(a, shift=0, pad=3):
    """a on the device as a view `shift` elements into a 16-byte aligned
    allocation pre-filled with the sentinel: -> (allocation, view)."""
    alloc = torch.from_numpy(np.full(a.size + shift + pad, C.SENTINEL, np.uint32).view(F)).to(DEV)
    v = alloc[shift:shift + a.size]
    v.copy_(torch.from_numpy(np.array(a)))
    assert alloc.data_ptr() % 16 == 0 and v.data_ptr() == alloc.data_ptr() + 4 * shift and v.is_contiguous()
    return alloc, v


def _sentinel(n):
    return np.full(n, C.SENTINEL, np.uint32).view(F)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _table(recs):
    from openfl_amd import lossy
    return lossy.LabelTable.from_rules(recs["start"], recs["end"], recs["mid"], recs["rank"], DEV)


@functools.lru_cache(maxsize=None)
def _want(name, rot, with_base):
    x, recs, base = C.apply_case(name, rot)
    out, inside = C.applied(x, recs, base if with_base else None)
    out.setflags(write=False)
    inside.setflags(write=False)
    return out, inside


def _where(got, want, recs):
    """The first differing element and its record, for a failure's message."""
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero((gn != wn) | ((got.view(np.uint32) != want.view(np.uint32)) & ~gn & ~wn))
    i = int(bad[0])
    t = np.flatnonzero((recs["start"] <= i) & (i < recs["end"]))
    return {"differ": bad.size, "first": i, "record": t.tolist(), "got": got[i], "want": want[i]}


def _apply(name, rot, with_base, shifts=(0, 0, 0)):
    """label_apply on one case, twice; x, base and out as views shifts[0..2]
    elements into their allocations.  Checks all the module docstring lists."""
    from openfl_amd import lossy
    x, recs, base = C.apply_case(name, rot)
    want, _ = _want(name, rot, with_base)
    xa, xd = _view(x, shifts[0])
    ba, bd = _view(base, shifts[1]) if with_base else (None, None)
    tab = _table(recs)
    runs = []
    for _ in range(2):
        oa, od = _view(_sentinel(x.size), shifts[2])
        assert lossy.label_apply(xd, tab, bd, od) is od
        runs.append(_bits(oa))
    assert np.array_equal(runs[0], runs[1])                                   # a second run is bit-identical
    so = shifts[2]
    got = runs[0][so:so + x.size].view(F)
    # inside the records the reference; outside them (want holds the sentinel there) nothing written
    assert C.same_bits(got, want) == 0, (name, rot, with_base, shifts, _where(got, want, recs))
    assert np.all(runs[0][:so] == C.SENTINEL) and np.all(runs[0][so + x.size:] == C.SENTINEL)
    sx = shifts[0]
    assert np.array_equal(_bits(xa)[sx:sx + x.size], x.view(np.uint32)) and np.all(_bits(xa)[:sx] == C.SENTINEL)
    if with_base:
        sb = shifts[1]
        assert np.array_equal(_bits(ba)[sb:sb + x.size], base.view(np.uint32)) and np.all(_bits(ba)[:sb] == C.SENTINEL)
    return got


# ---- a. label_apply against the reference -------------------------------------------
@pytest.mark.parametrize("rot", ROTS)
@pytest.mark.parametrize("name", C.APPLY_LAYOUTS)
def test_label_apply_designed(name, rot):
    """Every layout, with every rotation of the rules and value sets over its
    records, with a base and without."""
    x, recs, _ = C.apply_case(name, rot)
    if name == "counts/4160":   # the grid stride: more chunks than workgroups (two per CU)
        cus = torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count
        assert int(C.chunk_counts(recs).sum()) > 2 * cus
    _apply(name, rot, True)
    got = _apply(name, rot, False)
    want, inside = _want(name, rot, False)
    neg0 = want.view(np.uint32) == 0x80000000           # without a base a -0.0 value stays -0.0
    assert neg0.any() or not inside.any() or len(recs) < 8, name
    assert np.all(got.view(np.uint32)[neg0] == 0x80000000)


# ---- b. alignment ---------------------------------------------------------------------
@pytest.mark.parametrize("shifts", [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)],
                         ids=lambda s: "x%d_base%d_out%d" % s)
@pytest.mark.parametrize("name", ["short", "chunks"])
def test_label_apply_views_into_allocations(name, shifts):
    """x, base and out each 0 or 1 element into its allocation: only the two
    all-equal combinations take 16-byte accesses.  The allocations' elements
    around the views stay as they were (_apply)."""
    _apply(name, 0, True, shifts)
    if shifts[1] == 0:
        _apply(name, 1, False, shifts)


# ---- c. aliasing -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["counts/4097", "chunks"])
def test_label_apply_in_place(name):
    """out is base, and out is x_arena: the reference of the unmodified inputs
    inside the records, the input's own values outside them."""
    from openfl_amd import lossy
    x, recs, base = C.apply_case(name, 2)
    want, inside = _want(name, 2, True)
    tab = _table(recs)
    for alias, keep in (("base", base), ("x", x)):
        _, xd = _view(x)
        _, bd = _view(base)
        out = bd if alias == "base" else xd
        assert lossy.label_apply(xd, tab, bd, out) is out
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.uint32)[~inside], keep.view(np.uint32)[~inside]), (name, alias)
        merged = np.where(inside, want, got)
        assert C.same_bits(got[inside], want[inside]) == 0, (name, alias, _where(got, merged, recs))
        other = xd if alias == "base" else bd
        assert np.array_equal(_bits(other), (x if alias == "base" else base).view(np.uint32))


# ---- d. the ternary table -----------------------------------------------------------------
def _ternary_ref(x):
    """TernaryTransformer.forward (stc_pipeline.py:105-130; the mean of |x| in
    float64 from an exact sum, as the pipeline's statistics give it), then
    _float_to_int and the backward loop, in numpy:
    -> (int_to_float, (rank_neg, rank_zero, rank_pos), decoded float32)."""
    mean = math.fsum(np.abs(x.astype(np.float64))) / x.size
    out = np.where(x > 0.0, mean, 0.0)
    out = np.where(x < 0.0, -mean, out)
    uniq, ranks = np.unique(out, return_inverse=True)
    int_to_float = {i: u for i, u in enumerate(uniq)}
    r3 = tuple(float(np.flatnonzero(uniq == v)[0]) if np.any(uniq == v) else 0.0 for v in (-mean, 0.0, mean))
    if mean == 0.0:
        r3 = (0.0, 0.0, 0.0)
    return int_to_float, r3, C.chain_ref(ranks.astype(F), uniq)


def test_ternary_table_against_numpy():
    from openfl_amd import lossy
    tiny = np.finfo(F).tiny
    edge = np.array([0.0, -0.0, 1e-45, -1e-45, tiny, -tiny, np.nextafter(tiny, F(0)), -np.nextafter(tiny, F(0)),
                     3.0, -3.0, 0.25, -1e-3, 1e-40, -1e-40], F)
    rng = np.random.default_rng(23)
    cases = [np.tile(edge, 5), rng.permutation(np.tile(edge, 4700)),            # two chunks
             (rng.standard_normal(3001) * (rng.random(3001) < 0.1)).astype(F),
             np.abs(edge[edge != 0]), -np.abs(edge[edge != 0]), np.zeros(9, F), np.array([-0.0, 2.0, -0.0], F),
             np.array([-1e-45, 0.0], F)]
    starts, ends, total = C.placed([(c.size, t % 4, 3) for t, c in enumerate(cases)], lead=1)
    host = C.GAP_FILL[np.arange(total) % 4].copy()
    want = _sentinel(total)
    maps, r3 = [], []
    for s, c in zip(starts, cases):
        host[s:s + c.size] = c
        m, r, dec = _ternary_ref(c)
        maps.append(m)
        r3.append(r)
        want[s:s + c.size] = dec
    assert [len(m) for m in maps] == [3, 3, 3, 1, 1, 1, 2, 2]
    _, xd = _view(host)
    assert np.array_equal(_bits(xd), host.view(np.uint32))                      # -0.0 and denormals reach the device
    tab = lossy.ternary_label_table(starts, ends - starts, maps, r3, DEV)
    _, out = _view(_sentinel(total))
    lossy.label_apply(xd, tab, None, out)
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), _where(got, want, np.zeros(0, C.REC))
    first = got[starts[0]:starts[0] + edge.size]
    np.testing.assert_array_equal(first == 0, edge == 0)                        # only +-0.0 decode to 0
    np.testing.assert_array_equal(first < 0, edge < 0)                          # negative denormals included
    np.testing.assert_array_equal(first > 0, edge > 0)


# ---- e. value records of a fit ----------------------------------------------------------------
@pytest.mark.parametrize("value_f64", [False, True], ids=["f32", "f64"])
def test_value_records_follow_the_sequential_chain(value_f64):
    """Tensors of at most k distinct values: the fit returns them as uniq, so
    the map of the backward is designed -- a chain the whole table long, one
    that stops, values equal to earlier keys, none, and nuniq < k."""
    from openfl_amd import lossy
    xs = [C.chain_tensor(nm) for nm in C.CHAIN_NAMES]
    sizes = [x.size for x in xs]
    offs = [320 * t + 64 for t in range(len(xs))]      # 64-element aligned, as the round end lays its arenas out
    total = offs[-1] + 320
    assert all(n <= 256 for n in sizes)
    host = np.zeros(total, F)
    for o, x in zip(offs, xs):
        host[o:o + x.size] = x
    arena = torch.from_numpy(host).to(DEV)
    T = len(xs)
    ranks = torch.full_like(arena, -1.0)
    lab, val = lossy.LabelTable(T, DEV), lossy.LabelTable(T, DEV)
    uniq = lossy.kmeans_batch(arena, offs, sizes, C.CHAIN_K, n_init=6, seeds=[31 + 7 * t for t in range(T)],
                              value_f64=value_f64, ranks_out=ranks, label_out=lab, value_out=val)[3]
    lab_h, val_h = lab.buf.cpu().numpy().view(C.REC), val.buf.cpu().numpy().view(C.REC)
    ranks_h = ranks.cpu().numpy()
    _, out = _view(_sentinel(total))
    lossy.label_apply(arena, val, None, out)
    got = out.cpu().numpy()
    inside = np.zeros(total, bool)
    for t, (nm, o, x) in enumerate(zip(C.CHAIN_NAMES, offs, xs)):
        designed = np.array(C.CHAINS[nm], F)
        assert uniq[t].dtype == (np.float64 if value_f64 else F), nm
        assert np.array_equal(uniq[t], designed), (nm, uniq[t])
        np.testing.assert_array_equal(ranks_h[o:o + x.size], np.searchsorted(designed, x).astype(F), err_msg=nm)
        assert (val_h[t]["start"], val_h[t]["end"]) == (o, o + x.size) == (lab_h[t]["start"], lab_h[t]["end"])
        assert val_h[t]["mid"].tobytes() == lab_h[t]["mid"].tobytes(), nm
        # the value record: the reference's loop on the ranks of the label record
        assert val_h[t]["rank"].tobytes() == C.chain_ref(lab_h[t]["rank"], uniq[t]).tobytes(), \
            (nm, val_h[t]["rank"], lab_h[t]["rank"])
        want = C.chain_ref(ranks_h[o:o + x.size], uniq[t])
        assert got[o:o + x.size].tobytes() == want.tobytes(), nm
        inside[o:o + x.size] = True
        if nm == "full":
            assert np.all(want == 9.0)
        if nm == "earlier":
            assert np.array_equal(want, x)              # every value its own: nothing replaced a second time
    assert np.all(got.view(np.uint32)[~inside] == C.SENTINEL)
    assert np.all(ranks_h[~inside] == -1.0)


# ---- f. fused gzip labelling ----------------------------------------------------------------------
@pytest.mark.parametrize("one_off", [False, True], ids=["aligned", "one_off"])
@pytest.mark.parametrize("name", C.ENCODER_LAYOUTS)
def test_gzip_label_designed(name, one_off):
    """The stream of gzip_ranks(x, label=) decompresses to the reference's rank
    array (0 in every gap, whatever the gap holds) and equals byte for byte the
    stream of that rank array."""
    from openfl_amd import lossy
    x, recs = C.encoder_case(name, one_off)
    ref = C.ranks_of(x, recs)
    _, xd = _view(x, int(one_off))
    assert (xd.data_ptr() % 16 == 0) == (not one_off)
    tab = _table(recs)
    z = lossy.gzip_ranks(xd, label=tab)
    raw = np.frombuffer(gzip.decompress(z), F)
    assert raw.size == ref.size
    bad = np.flatnonzero(raw.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, (name, bad.size, int(bad[0]), raw[bad[0]], ref[bad[0]])
    assert z == lossy.gzip_ranks(torch.from_numpy(ref).to(DEV))
    assert z == lossy.gzip_ranks(xd, label=tab)


@pytest.mark.parametrize("bad", (32.0, 2.5))
def test_gzip_label_refuses_a_bad_rank(bad):
    """A record whose rank 32.0 (2.5) an element takes is refused like such a
    value in a rank array, and the call made after it is unaffected."""
    from openfl_amd import lossy
    from openfl_amd._lib import CodecError
    x, recs = C.encoder_case("single")
    _, xd = _view(x)
    good = _table(recs)
    z = lossy.gzip_ranks(xd, label=good)
    with pytest.raises(CodecError):
        lossy.gzip_ranks(xd, label=_table(C.refused_case(bad)[1]))
    assert lossy.gzip_ranks(xd, label=good) == z
    assert gzip.decompress(z) == C.ranks_of(x, recs).tobytes()
