"""Decode fused with the streaming average (EdenPlan.decode_accumulate,
k_dec_acc_rowC / k_dec_acc_rowC2, WavgAccumulator.add_upload(fused=True)).

The reference is plan.decode(..., base=base) into y_c and then, in torch on
the device, s = y_0.double() * w_0; s = s + y_1.double() * w_1; ... -- the
same IEEE operations in the same order, so every comparison is torch.equal on
the tensors' ranges; no tolerance is involved.  sums and y_small start as NaN:
a first call that added instead of storing, or a large slice that went through
y, would show.  The file takes about 3 s on an MI355X.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

BATCH = [5, 1000, 4096, 70_000, 1 << 20, 3]
W = [0.2, 0.3, 0.5]
IDS = lambda v: "_".join(map(str, v)) if isinstance(v, list) else str(v)  # noqa: E731
# numels, bits, plan knobs
PLANS = [([1 << 16], 8, {}), ([1 << 16], 3, {}), ([1 << 18], 8, {}), ([120_003], 8, {}),
         ([(1 << 23) + 70_001], 8, {}), ([1 << 25], 8, {}), ([1 << 26], 8, {}), (BATCH, 8, {}),
         (BATCH, 8, {"wave_mib": 0.5}), ([1 << 18], 8, {"row2": 0}), ([1 << 18], 8, {"row2": 1}),
         ([1 << 20], 8, {"pair": 1})]
ROW_TILE = 1 << 15


def _nan(n, dtype):
    return torch.full((n,), float("nan"), dtype=dtype, device=DEV)


def _uploads(plan, n, std=0.02):
    """n collaborators' planes and scales from plan.encode of normal arenas -> (seeds, [(planes, scales)], ws)."""
    g = torch.Generator(device=DEV).manual_seed(7)
    sd = torch.arange(100, 100 + len(plan.numels), dtype=torch.int32, device=DEV)
    ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
    ups = []
    for _ in range(n):
        x = torch.empty(plan.arena_numel, device=DEV).normal_(0, std, generator=g)
        planes = torch.empty(max(plan.planes_bytes, 1), dtype=torch.uint8, device=DEV)
        scales = torch.empty(plan.n_slices, device=DEV)
        plan.encode(x, sd, planes, scales, ws)
        ups.append((planes, scales))
    return sd, ups, ws


@pytest.mark.parametrize("with_base", [True, False], ids=["base", "nobase"])
@pytest.mark.parametrize("numels,bits,knobs", PLANS, ids=IDS)
def test_sums_are_accumulate_of_decode(numels, bits, knobs, with_base):
    from openfl_amd import _lib
    from openfl_amd.aggregation import _RangeTable
    from openfl_amd.codec import EdenPlan, slice_plan
    plan = EdenPlan(numels, bits, **knobs)
    slices = []   # (start, valid elements, P) of every slice, in arena order
    for t, (o, n) in enumerate(zip(plan.elem_offsets, numels)):
        for P, ln in zip(plan.dims[t], slice_plan(n)[1]):
            slices.append((o, ln, P))
            o += ln
    small = _RangeTable([(o, ln) for o, ln, P in slices if P <= ROW_TILE and ln], DEV)   # the caller's to fold
    st = torch.cuda.current_stream(DEV).cuda_stream
    assert "wave_mib" not in knobs or plan.n_waves > 1
    names = [l["name"] for l in plan.accumulate_launches()]
    assert not {"ofl::k_dec_rowC", "ofl::k_dec_rowC2"} & set(names)
    if "row2" in knobs:
        assert ("ofl::k_dec_acc_rowC2" in names) == bool(knobs["row2"]) and ("ofl::k_dec_acc_rowC" in names) != bool(knobs["row2"])
    sd, ups, ws = _uploads(plan, len(W))
    base = torch.empty(plan.arena_numel, device=DEV).normal_(0, 1.0, generator=torch.Generator(device=DEV).manual_seed(8)) \
        if with_base else None
    sums, y_small, want = _nan(plan.arena_numel, torch.float64), _nan(plan.arena_numel, torch.float32), None
    for c, (planes, scales) in enumerate(ups):
        y = _nan(plan.arena_numel, torch.float32)
        plan.decode(planes, sd, scales, y, ws, base=base)
        want = y.double() * W[0] if c == 0 else want + y.double() * W[c]
        plan.decode_accumulate(planes, sd, scales, sums, W[c], c == 0, y_small, ws, base=base)
        _lib.check_agg(_lib.lib().ofl_wavg_accumulate_ranges(y_small.data_ptr(), W[c], 1 if c == 0 else 0, *small.args,
                                                             sums.data_ptr(), st))
    torch.cuda.synchronize()
    for o, ln, P in slices:
        r = slice(o, o + ln)
        assert torch.equal(sums[r], want[r]) and not want[r].isnan().any(), (o, P)
        if P > ROW_TILE:
            assert y_small[r].isnan().all(), (o, P)   # never went through y
        else:
            assert torch.equal(y_small[r], y[r]), (o, P)
    used = torch.zeros(plan.arena_numel, dtype=torch.bool, device=DEV)
    for o, ln, _ in slices:
        used[o:o + ln] = True
    assert sums[~used].isnan().all()   # no alignment gap, nothing at or past a tensor's length


def test_negative_zero_first_product_is_stored():
    from openfl_amd.codec import EdenPlan
    plan = EdenPlan([1 << 16], 8)
    sd, ((planes, scales),), ws = _uploads(plan, 1, std=0.0)   # planes of zeros, scale 0
    assert not scales.any()
    zeros = torch.zeros(plan.arena_numel, device=DEV)
    # decoded zeros carry the D1 signs, so without a base the sums' signs are
    # those of -y; with a base of +0.0, x = +0.0 + (+-0.0) = +0.0 and every
    # first product is -0.0
    for base in (zeros, None):
        y, sums = _nan(plan.arena_numel, torch.float32), _nan(plan.arena_numel, torch.float64)
        plan.decode(planes, sd, scales, y, ws, base=base)
        plan.decode_accumulate(planes, sd, scales, sums, -1.0, True, None, ws, base=base)
        assert not sums.any() and torch.equal(sums.signbit(), (y.double() * -1.0).signbit())
        assert base is None or sums.signbit().all()
        plan.decode_accumulate(planes, sd, scales, sums, 1.0, False, None, ws, base=base)
        assert not sums.any() and not sums.signbit().any()


SHAPES = [(300,), (70_000,), (1 << 16,), (50,), (1,), (1 << 18,)]


def _round_inputs(re, pipe):
    rng = np.random.default_rng(3)
    base = re.pack([rng.standard_normal(s).astype(np.float32) for s in SHAPES])
    uploads = [[pipe.forward(rng.standard_normal(s).astype(np.float32) * np.float32(0.02)) for s in SHAPES]
               for _ in W]
    return base, uploads


@pytest.mark.parametrize("delta", [True, False])
def test_add_upload_fused_equals_unfused(delta):
    from openfl_amd.aggregation import RoundEnd
    from openfl_amd.pipelines.eden_pipeline import EdenPipeline
    pipe = EdenPipeline(n_bits=8, device=DEV, seed_mode="fast")
    re = RoundEnd(pipe, SHAPES, DEV)
    base, uploads = _round_inputs(re, pipe)
    got = {}
    for fused in (False, True):
        acc = re.accumulator(sums=_nan(re.arena_numel, torch.float64))
        for items, w in zip(uploads, W):
            acc.add_upload(items, w, delta=delta, base_arena=base if delta else None, fused=fused)
        sums = acc.sums.clone()
        np.random.seed(11)
        got[fused] = (sums,) + tuple(re.finish(acc, base_arena=base))
    (s0, m0, p0, sd0), (s1, m1, p1, sd1) = got[False], got[True]
    from tests.round_stream_cases import md_key
    assert torch.as_tensor(sd0).tolist() == torch.as_tensor(sd1).tolist()
    for i, (o, n) in enumerate(zip(re.offsets, re.numels)):
        assert torch.equal(s0[o:o + n], s1[o:o + n]) and not s0[o:o + n].isnan().any(), i
        assert torch.equal(re.view(m0, i), re.view(m1, i)), i
        assert p0[i][0] == p1[i][0] and md_key(p0[i][1]) == md_key(p1[i][1]), i


def test_add_upload_fused_refuses_what_it_cannot_take():
    from openfl_amd._lib import CodecError
    from openfl_amd.aggregation import RoundEnd
    from openfl_amd.pipelines import KCPipeline, NoCompressionPipeline
    from openfl_amd.pipelines.eden_pipeline import EdenPipeline
    pipe = EdenPipeline(n_bits=8, device=DEV, seed_mode="fast")
    rng = np.random.default_rng(5)
    xs = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    nc = NoCompressionPipeline()
    for re, items, lossless in ((RoundEnd(pipe, SHAPES, DEV), [nc.forward(x) for x in xs], True),
                                (RoundEnd(KCPipeline(device=DEV), SHAPES, DEV), [], False)):
        acc = re.accumulator(sums=_nan(re.arena_numel, torch.float64))
        with pytest.raises(CodecError, match="fused=True"):
            acc.add_upload(items, 1.0, lossless=lossless, delta=False, fused=True)
        torch.cuda.synchronize()
        assert acc.sums.isnan().all() and acc.weights == []


@pytest.mark.parametrize("null", ["sums", "y_small"])
def test_c_call_refuses_null_arguments(null):
    from openfl_amd import _lib
    from openfl_amd.codec import EdenPlan
    plan = EdenPlan([1 << 16, 1000], 8)   # 1000: a slice of at most 2^15 elements
    sd, ((planes, scales),), ws = _uploads(plan, 1)
    sums, y_small = _nan(plan.arena_numel, torch.float64), _nan(plan.arena_numel, torch.float32)
    ptr = {"sums": sums.data_ptr(), "y_small": y_small.data_ptr(), null: None}
    rc = _lib.lib().ofl_eden_decode_accumulate(plan.handle, planes.data_ptr(), sd.data_ptr(), scales.data_ptr(), None,
                                               ctypes.c_double(1.0), 1, ptr["sums"], ptr["y_small"], ws.data_ptr(),
                                               ws.numel(), torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.OFL_EINVAL
    assert sums.isnan().all() and y_small.isnan().all()
