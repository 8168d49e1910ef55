"""Decode fused with the FedOpt gradient (EdenPlan.decode_adaptive_accumulate,
k_dec_ada_rowC / k_dec_ada_rowC2, ofl_adaptive_accumulate_ranges,
AdaptiveAccumulator.add_upload(fused=True)).

The reference is plan.decode(..., base=base if delta else None) into y and
then, in torch float32 on the device, t = w32 * (base - y); g = 0 + t on the
first upload, g = g + t on later ones -- the same IEEE operations in the same
order, so every comparison is torch.equal on the tensors' ranges; no tolerance
is involved.  g and y_small start as NaN: a first call that added instead of
storing, or a large slice that went through y, would show.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_eden_decode_accumulate import BATCH, DEV, IDS, ROW_TILE, SHAPES, _nan, _round_inputs, _uploads

pytestmark = pytest.mark.gpu

W32 = [float(np.float32(w)) for w in (0.2, -0.3, 0.5)]
# numels, bits, plan knobs
PLANS = [([1 << 16], 8, {}), ([1 << 16], 3, {}), ([1 << 18], 8, {"row2": 0}), ([1 << 18], 8, {"row2": 1}),
         ([120_003], 8, {}), ([1 << 20], 8, {"pair": 1}), (BATCH, 8, {}), (BATCH, 8, {"wave_mib": 0.5}),
         ([1 << 26], 8, {})]


def _base(n, seed=8):
    return torch.empty(n, device=DEV).normal_(0, 1.0, generator=torch.Generator(device=DEV).manual_seed(seed))


@pytest.mark.parametrize("delta", [True, False], ids=["delta", "nodelta"])
@pytest.mark.parametrize("numels,bits,knobs", PLANS, ids=IDS)
def test_gradient_is_accumulate_of_decode(numels, bits, knobs, delta):
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
    names = {l["name"] for l in plan.adaptive_launches()}
    assert not {"ofl::k_dec_rowC", "ofl::k_dec_rowC2"} & names
    assert names & {"ofl::k_dec_ada_rowC", "ofl::k_dec_ada_rowC2"}
    if "row2" in knobs:
        assert ("ofl::k_dec_ada_rowC2" in names) == bool(knobs["row2"]) and ("ofl::k_dec_ada_rowC" in names) != bool(knobs["row2"])
    sd, ups, ws = _uploads(plan, len(W32))
    base = _base(plan.arena_numel)
    g, y_small, want = _nan(plan.arena_numel, torch.float32), _nan(plan.arena_numel, torch.float32), None
    for c, (planes, scales) in enumerate(ups):
        y = _nan(plan.arena_numel, torch.float32)
        plan.decode(planes, sd, scales, y, ws, base=base if delta else None)
        t = W32[c] * (base - y)
        want = 0 + t if c == 0 else want + t
        plan.decode_adaptive_accumulate(planes, sd, scales, g, W32[c], c == 0, y_small, ws, base=base, delta=delta)
        _lib.check_agg(_lib.lib().ofl_adaptive_accumulate_ranges(y_small.data_ptr(), W32[c], base.data_ptr(),
                                                                 1 if c == 0 else 0, *small.args, g.data_ptr(), st))
    torch.cuda.synchronize()
    for o, ln, P in slices:
        r = slice(o, o + ln)
        assert torch.equal(g[r], want[r]) and not want[r].isnan().any(), (o, P)
        if P > ROW_TILE:
            assert y_small[r].isnan().all(), (o, P)   # never went through y
        else:
            assert torch.equal(y_small[r], y[r]), (o, P)
    used = torch.zeros(plan.arena_numel, dtype=torch.bool, device=DEV)
    for o, ln, _ in slices:
        used[o:o + ln] = True
    assert g[~used].isnan().all()   # no alignment gap, nothing at or past a tensor's length


def test_first_add_is_kept():
    from openfl_amd.codec import EdenPlan
    plan = EdenPlan([1 << 16], 8)
    sd, ((planes, scales),), ws = _uploads(plan, 1, std=0.0)   # planes of zeros, scale 0
    assert not scales.any()
    zeros = torch.zeros(plan.arena_numel, device=DEV)
    # x = +0.0 + (+-0.0) = +0.0, base - x = +0.0 and the product with -1 is -0.0:
    # +0.0f + -0.0 is +0.0, where a stored product would leave the sign bit
    g = _nan(plan.arena_numel, torch.float32)
    plan.decode_adaptive_accumulate(planes, sd, scales, g, -1.0, True, None, ws, base=zeros, delta=True)
    assert not g.any() and not g.signbit().any()


def _opt_bits(re):
    st = re.optimizer_state()
    return [st["step"]] + [None if t is None else [re.view(t, i).cpu().numpy().tobytes() for i in range(len(SHAPES))]
                           for t in (st["params"], st["first_moment"], st["second_moment"])]


@pytest.mark.parametrize("delta", [True, False])
@pytest.mark.parametrize("kind", ["adam", "adagrad"])
def test_add_upload_fused_equals_unfused(kind, delta):
    from openfl_amd._lib import CodecError
    from openfl_amd.aggregation import RoundEnd
    from openfl_amd.pipelines.eden_pipeline import EdenPipeline
    from tests.round_stream_cases import md_key
    pipe = EdenPipeline(n_bits=8, device=DEV, seed_mode="fast")
    got, base = {}, None
    # fused None with a base_arena of other storage takes the unfused route
    for fused, own_base in ((False, True), (True, True), (None, False)):
        re = RoundEnd(pipe, SHAPES, DEV, aggregation=kind)   # one each: finish() moves the optimiser state
        if base is None:
            base, uploads = _round_inputs(re, pipe)
        re.init_optimizer(base)
        acc = re.accumulator(sums=_nan(re.arena_numel, torch.float32), base_arena=base)
        up_base = base if own_base else base.clone()
        if not own_base and delta:
            with pytest.raises(CodecError, match="fused=True"):
                acc.add_upload(uploads[0], W32[0], delta=True, base_arena=up_base, fused=True)
            torch.cuda.synchronize()
            assert acc.sums.isnan().all() and acc.weights == []
        for items, w in zip(uploads, W32):
            acc.add_upload(items, w, delta=delta, base_arena=up_base if delta else None, fused=fused)
        sums = acc.sums.clone()
        np.random.seed(11)
        got[fused] = (sums,) + tuple(re.finish(acc, base_arena=base)) + (_opt_bits(re), re)
    s0, m0, p0, sd0, o0, re = got[False]
    for s1, m1, p1, sd1, o1, _ in (got[True], got[None]):
        assert torch.as_tensor(sd0).tolist() == torch.as_tensor(sd1).tolist() and o0 == o1
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
    for re, items, lossless in ((RoundEnd(pipe, SHAPES, DEV, aggregation="adam"), [nc.forward(x) for x in xs], True),
                                (RoundEnd(KCPipeline(device=DEV), SHAPES, DEV, aggregation="adam"), [], False)):
        base = re.pack(xs)
        re.init_optimizer(base)
        acc = re.accumulator(sums=_nan(re.arena_numel, torch.float32), base_arena=base)
        with pytest.raises(CodecError, match="fused=True"):
            acc.add_upload(items, 1.0, lossless=lossless, delta=False, fused=True)
        torch.cuda.synchronize()
        assert acc.sums.isnan().all() and acc.weights == []


@pytest.mark.parametrize("null", ["g", "base", "y_small"])
def test_c_call_refuses_null_arguments(null):
    from openfl_amd import _lib
    from openfl_amd.codec import EdenPlan
    plan = EdenPlan([1 << 16, 1000], 8)   # 1000: a slice of at most 2^15 elements
    sd, ((planes, scales),), ws = _uploads(plan, 1)
    g, y_small, base = _nan(plan.arena_numel, torch.float32), _nan(plan.arena_numel, torch.float32), _base(plan.arena_numel)
    ptr = {"g": g.data_ptr(), "base": base.data_ptr(), "y_small": y_small.data_ptr(), null: None}
    rc = _lib.lib().ofl_eden_decode_adaptive_accumulate(
        plan.handle, planes.data_ptr(), sd.data_ptr(), scales.data_ptr(), ptr["base"], 1, ctypes.c_float(1.0), 1,
        ptr["g"], ptr["y_small"], ws.data_ptr(), ws.numel(), torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.OFL_EINVAL
    assert g.isnan().all() and y_small.isnan().all()
