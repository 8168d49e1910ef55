"""GPU: the weighted average one collaborator at a time.

ofl_wavg_accumulate / ofl_wavg_finish against NumPy bit for bit (np.average
of the stack, generate_delta's float64 subtraction, its float32 rounding), on
arenas as allocated (16-byte bodies) and on views one element into a larger
tensor (scalar bodies), and against ofl_wavg_delta on the same inputs;
RoundEnd.accumulator / add / finish against run() on the same arenas and weights: model bits, payload bytes, metadata, seeds and
the np.random state, for the Eden pipeline in both seed modes and the KC, SKC
and STC pipelines; and the accumulator's errors, each raised before anything
is drawn from np.random."""
import functools
import gzip

import numpy as np
import pytest
import torch

from tests.round_stream_cases import (DEV, F, PIPELINES, SHAPES, SHAPES_ROW, bits, make_pipeline, md_key, rng_state,
                                      shapes_for, tensors)

pytestmark = pytest.mark.gpu
SENTINEL = 123.25
WEIGHTS = [2.5, 0.0, 1.0, 0.375, 7.0]   # not normalised; a zero among them


def _weights(C):
    return np.asarray([WEIGHTS[c % len(WEIGHTS)] + (c // len(WEIGHTS)) for c in range(C)], np.float64)


def _stack(C, n):
    """C rows of n float32 values with -0.0, denormals and +-3e38 among them;
    column 0 is -0.0 in every row."""
    rng = np.random.default_rng(100 * C + n)
    x = (rng.standard_normal((C, n)) * 0.1).astype(F)
    special = np.array([-0.0, 1e-45, -1e-40, 3e38, -3e38, 1.1754942e-38], F)
    x[rng.integers(0, C, 4 * C), rng.integers(0, n, 4 * C)] = special[rng.integers(0, special.size, 4 * C)]
    x[:, 0] = F(-0.0)
    if C > 1:
        x[1, 1] = F(3e38)   # times the zero weight
    return x


def _dev(host, offset, dtype=None):
    """A device copy of host: as allocated, or the view one element into a
    larger tensor (aligned to the element only), with a sentinel after it."""
    t = torch.from_numpy(np.ascontiguousarray(host))
    big = torch.full((offset + t.numel() + 3,), SENTINEL, dtype=t.dtype, device=DEV)
    big[offset:offset + t.numel()] = t.to(DEV)
    return big, big[offset:offset + t.numel()]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", [5, 64, 1027])
@pytest.mark.parametrize("C", [1, 2, 3, 16, 17, 33])
def test_accumulate_and_finish_equal_numpy(C, n, offset):
    from openfl_amd import _lib
    from openfl_amd.aggregation import _wavg_launch, weight_sum
    L = _lib.lib()
    x, w = _stack(C, n), _weights(C)
    want = np.average(x, weights=w, axis=0)
    assert want.dtype == np.float64
    # a column whose products are all -0.0: the kernels keep the first product, so the sum is -0.0 (the rule
    # ofl_wavg_delta has, and what run() computes); NumPy 2 starts its add reduction from +0.0 and gives +0.0
    prod = x.astype(np.float64) * w[:, None]
    want[np.all((prod == 0.0) & np.signbit(prod), axis=0)] = -0.0
    assert np.signbit(want[0]) and want[0] == 0.0
    wsum = weight_sum(w, 1)
    st = torch.cuda.current_stream().cuda_stream
    base_h = (np.random.default_rng(n).standard_normal(n) * 0.1).astype(F)
    base_h[0] = F(0.0)
    for base in (None, base_h):
        sums_big, sums = _dev(np.full(n, SENTINEL, np.float64), offset)
        keep = []
        for c in range(C):
            xb, xv = _dev(x[c], offset)
            keep.append(xb)
            _lib.check_agg(L.ofl_wavg_accumulate(xv.data_ptr(), float(w[c]), 1 if c == 0 else 0, n, sums.data_ptr(), st))
        d64_big, d64 = _dev(np.full(n, SENTINEL, np.float64), offset)
        d32_big, d32 = _dev(np.full(n, SENTINEL, F), offset)
        bb, bv = _dev(base, offset) if base is not None else (None, None)
        _lib.check_agg(L.ofl_wavg_finish(sums.data_ptr(), wsum, bv.data_ptr() if bv is not None else None, n,
                                         d64.data_ptr(), d32.data_ptr(), st))
        torch.cuda.synchronize()
        delta = want - base if base is not None else want
        assert bits(sums.cpu().numpy()) == bits(want)
        assert bits(d64.cpu().numpy()) == bits(delta)
        assert bits(d32.cpu().numpy()) == bits(delta.astype(F))
        for big in (sums_big, d64_big, d32_big):   # nothing outside [offset, offset + n)
            assert (big[:offset] == SENTINEL).all() and (big[offset + n:] == SENTINEL).all()
        # the file's one-launch kernel on the same inputs: the same bits everywhere
        xs = [kb[offset:offset + n] for kb in keep]
        p_agg, p64, p32 = (_dev(np.full(n, SENTINEL, t), offset)[1] for t in (np.float64, np.float64, F))
        _wavg_launch(xs, w, wsum, bv, n, agg=p_agg, delta64=p64, delta32=p32, device=torch.device(DEV))
        for got, parent in ((sums, p_agg), (d64, p64), (d32, p32)):
            assert bits(got.cpu().numpy()) == bits(parent.cpu().numpy())


def test_finish_writes_only_what_is_asked_for():
    from openfl_amd import _lib
    L = _lib.lib()
    n = 1027
    x = _stack(1, n)[0]
    st = torch.cuda.current_stream().cuda_stream
    _, xv = _dev(x, 0)
    _, sums = _dev(np.zeros(n, np.float64), 0)
    _lib.check_agg(L.ofl_wavg_accumulate(xv.data_ptr(), 3.0, 1, n, sums.data_ptr(), st))
    _lib.check_agg(L.ofl_wavg_finish(sums.data_ptr(), 3.0, None, n, None, None, st))
    assert bits(sums.cpu().numpy()) == bits(x.astype(np.float64) * 3.0 / 3.0)
    assert L.ofl_wavg_finish(sums.data_ptr(), 3.0, None, n, sums.data_ptr(), None, st) == _lib.OFL_EINVAL
    assert L.ofl_wavg_accumulate(None, 1.0, 1, n, sums.data_ptr(), st) == _lib.OFL_EINVAL
    assert L.ofl_wavg_accumulate(xv.data_ptr(), 1.0, 1, 0, None, st) == _lib.OFL_OK


# ------------------------------------------------------------- streaming against run() ---
@functools.lru_cache(maxsize=None)
def _round_end(name, shapes=tuple(SHAPES), aggregation="weighted_average"):
    from openfl_amd.aggregation import RoundEnd
    return RoundEnd(make_pipeline(name), list(shapes), device=DEV, aggregation=aggregation)


@functools.lru_cache(maxsize=None)
def _inputs(C, shapes=tuple(SHAPES)):
    """The base model and C collaborators' tensors (host); shared, never modified."""
    base = tensors(shapes, 7, 0.1)
    collabs = [[b + d for b, d in zip(base, tensors(shapes, 1000 + c))] for c in range(C)]
    return base, collabs


def _arenas(re, C):
    base, collabs = _inputs(C, tuple(re.shapes))
    return re.pack(base), [re.pack(c) for c in collabs]


def _same_payloads(re, got, want, lossy):
    assert (got is None) == (want is None)
    if got is None:
        return
    assert len(got) == len(want)
    for i, ((pg, mg), (pw, mw)) in enumerate(zip(got, want)):
        if lossy and re.numels[i] < 6 and pg != pw:   # the host gzip's header carries a time stamp
            assert gzip.decompress(pg) == gzip.decompress(pw), i
        else:
            assert pg == pw, i
        assert md_key(mg) == md_key(mw), i


def _seed_list(s):
    return s.cpu().tolist() if isinstance(s, torch.Tensor) else list(s)


@pytest.mark.parametrize("payloads", [True, False], ids=["payloads", "nopayloads"])
@pytest.mark.parametrize("with_base", [True, False], ids=["base", "nobase"])
@pytest.mark.parametrize("C", [3, 18])
@pytest.mark.parametrize("name", PIPELINES)
def test_streaming_equals_run(name, C, with_base, payloads):
    re = _round_end(name, shapes_for(name))
    base, xs = _arenas(re, C)
    base = base if with_base else None
    w = [float(v) for v in _weights(C)]
    np.random.seed(31)
    m1, p1, s1 = re.run(xs, w, base, payloads=payloads)
    m1, s1, after1 = m1.cpu().numpy(), _seed_list(s1), rng_state()
    np.random.seed(31)
    acc = re.accumulator()
    for x, wc in zip(xs, w):
        acc.add(x, wc)
    m2, p2, s2 = re.finish(acc, base_arena=base, payloads=payloads)
    assert bits(m2.cpu().numpy()) == bits(m1)
    assert _seed_list(s2) == s1
    assert rng_state() == after1
    _same_payloads(re, p2, p1, not name.startswith("eden"))


@pytest.mark.parametrize("name", ["eden_ref", "eden_fast"])
def test_streaming_equals_run_with_a_row_pass_slice(name):
    re = _round_end(name, tuple(SHAPES_ROW))
    assert any(P > 1 << 15 for d in re.plan.dims for P in d)
    base, xs = _arenas(re, 3)
    w = [0.5, 2.0, 1.25]
    np.random.seed(5)
    m1, p1, s1 = re.run(xs, w, base)
    after1 = rng_state()
    np.random.seed(5)
    acc = re.accumulator()
    for x, wc in zip(xs, w):
        acc.add(x, wc)
    m2, p2, s2 = re.finish(acc, base_arena=base)
    assert bits(m2.cpu().numpy()) == bits(m1.cpu().numpy()) and s2 == s1 and rng_state() == after1
    _same_payloads(re, p2, p1, False)


@pytest.mark.parametrize("C", [3, 18])
def test_agg_out_equals_runs(C):
    re = _round_end("eden_fast")
    base, xs = _arenas(re, C)
    w = [float(v) for v in _weights(C)]
    a1 = torch.full((re.arena_numel,), SENTINEL, dtype=torch.float64, device=DEV)
    np.random.seed(2)
    m1 = re.run(xs, w, base, agg_out=a1, payloads=False)[0]
    # a separate agg_out: the average lands in both
    a2 = torch.full_like(a1, SENTINEL)
    np.random.seed(2)
    acc = re.accumulator()
    for x, wc in zip(xs, w):
        acc.add(x, wc)
    m2 = re.finish(acc, base_arena=base, agg_out=a2, payloads=False)[0]
    assert bits(a2.cpu().numpy()) == bits(a1.cpu().numpy()) == bits(acc.sums.cpu().numpy())
    assert bits(m2.cpu().numpy()) == bits(m1.cpu().numpy())
    # the caller's sums arena is agg_out itself
    a3 = torch.full_like(a1, SENTINEL)
    np.random.seed(2)
    acc = re.accumulator(sums=a3)
    assert acc.sums is a3
    for x, wc in zip(xs, w):
        acc.add(x, wc)
    re.finish(acc, base_arena=base, agg_out=a3, payloads=False)
    assert bits(a3.cpu().numpy()) == bits(a1.cpu().numpy())


def test_single_elements_follow_numpys_pairwise_order():
    """18 collaborators: NumPy sums a (18, 1) stack with eight accumulators,
    not in order; the table keeps every collaborator's element for that."""
    re = _round_end("eden_fast")
    C = 18
    base, collabs = _inputs(C)
    _, xs = _arenas(re, C)
    w = _weights(C)
    acc = re.accumulator()
    for x, wc in zip(xs, w):
        acc.add(x, float(wc))
    agg = torch.empty(re.arena_numel, dtype=torch.float64, device=DEV)
    re.finish(acc, agg_out=agg, payloads=False)
    agg = agg.cpu().numpy()
    for i, shape in enumerate(SHAPES):
        want = np.average([c[i] for c in collabs], weights=w, axis=0)
        o = re.offsets[i]
        assert bits(agg[o:o + re.numels[i]]) == bits(want), i


def test_add_upload_of_a_lossless_upload_equals_add_of_its_ingest():
    from openfl_amd.pipelines import NoCompressionPipeline
    re = _round_end("eden_fast")
    C = 3
    base, collabs = _inputs(C)
    base_a, xs = _arenas(re, C)
    nc = NoCompressionPipeline()
    uploads = [[nc.forward(t) for t in c] for c in collabs]
    w = [1.0, 4.0, 0.5]
    results = []
    for mode in ("run", "add", "add_upload"):
        np.random.seed(77)
        if mode == "run":
            results.append(re.run(xs, w, base_a))
            continue
        acc = re.accumulator()
        for items, wc in zip(uploads, w):
            if mode == "add":
                acc.add(re.ingest(items, lossless=True, delta=False), wc)
            else:
                acc.add_upload(items, wc, lossless=True, delta=False)
        results.append(re.finish(acc, base_arena=base_a))
    for m, p, s in results[1:]:
        assert bits(m.cpu().numpy()) == bits(results[0][0].cpu().numpy()) and s == results[0][2]
        _same_payloads(re, p, results[0][1], False)


def test_weight_rules_are_runs():
    re = _round_end("eden_fast")
    _, xs = _arenas(re, 3)
    before = rng_state()
    acc = re.accumulator()
    for x in xs[:2]:
        acc.add(x, 0.0)
    with pytest.raises(ZeroDivisionError):
        re.finish(acc)
    from openfl_amd._lib import CodecError
    with pytest.raises(CodecError, match="float64"):
        re.accumulator().add(xs[0], np.float32(1.0))
    assert rng_state() == before


def test_accumulator_errors_come_before_any_draw():
    from openfl_amd._lib import CodecError
    re = _round_end("eden_fast")
    _, xs = _arenas(re, 3)
    np.random.seed(9)
    before = rng_state()
    with pytest.raises(CodecError, match="weighted average"):
        _round_end("eden_fast", aggregation="median").accumulator()
    with pytest.raises(CodecError, match="without an add"):
        re.finish(re.accumulator())
    acc = re.accumulator()
    for bad in (xs[0].double(), xs[0][:re.arena_numel - 1], xs[0].cpu(), xs[0][::2]):
        with pytest.raises(CodecError, match="arenas must be"):
            acc.add(bad, 1.0)
    assert acc.weights == []
    with pytest.raises(CodecError, match="arenas must be"):
        acc.add(xs[0], 1.0)
        re.finish(acc, base_arena=xs[1].double())
    with pytest.raises(CodecError, match="of this RoundEnd"):
        _round_end("eden_ref").finish(acc)
    with pytest.raises(CodecError, match="agg_out"):
        re.finish(acc, agg_out=torch.empty(re.arena_numel, dtype=torch.float32, device=DEV))
    assert rng_state() == before and not acc.finished
    re.finish(acc, payloads=False)
    after = rng_state()
    assert after != before
    with pytest.raises(CodecError, match="after finish"):
        acc.add(xs[0], 1.0)
    with pytest.raises(CodecError, match="after finish"):
        acc.add_upload([], 1.0)
    with pytest.raises(CodecError, match="after finish"):
        re.finish(acc)
    assert rng_state() == after
