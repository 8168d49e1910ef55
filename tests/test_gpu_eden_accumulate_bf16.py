"""The weighted average's streaming round on bfloat16 model arenas
(ofl_eden_decode_accumulate_bf16, csrc/eden_dec_acc_bf16.h; the bf16 forms in
agg_kernels.hip; RoundEnd.accumulator / add / add_upload / finish), held to the
float32 round of the same library on the widened base, which the other GPU
tests hold to NumPy and the oracle.  A bf16 base stands for its exact float32
widening, so everything is bit for bit (integer views) and the new model is the
float32 model rounded once, as torch's .to(torch.bfloat16) rounds.

NUMELS are tests/test_gpu_eden_bf16.py's: quad tails of 1 and 3, a tile without
a valid element, large + small + tiny slices in one tensor, small-only tensors;
row2=0 runs the persistent kernel, pair=1 the paired table, one 2^26 slice at
64 MiB waves the explicit paired tile lists."""
import functools

import numpy as np
import pytest
import torch

from tests.round_stream_cases import md_key
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

NUMELS = [60001, 125003, 480001, 98311, 4099, 101, 7]
PLANS = [(NUMELS, 8, {}), (NUMELS, 3, {}), (NUMELS, 8, {"row2": 0}), (NUMELS, 8, {"pair": 1}),
         ([1 << 26], 8, {"wave_mib": 64, "streams": 1})]
IDS = ["8b", "3b", "row2_0", "pair_1", "split"]
W = [0.2, 0.3, 0.5]
SHAPES = [(300,), (70_000,), (1 << 16,), (50,), (1,), (1 << 18,)]


def _nan(n, dtype):
    return torch.full((n,), float("nan"), dtype=dtype, device=DEV)


@pytest.mark.parametrize("with_base", [True, False], ids=["base", "nobase"])
@pytest.mark.parametrize("numels,bits,knobs", PLANS, ids=IDS)
def test_sums_equal_the_widened_float32_fold(numels, bits, knobs, with_base):
    from openfl_amd.codec import EdenPlan
    plan = EdenPlan(numels, bits, **knobs)
    n = plan.arena_numel
    used = torch.zeros(n, dtype=torch.bool, device=DEV)
    for o, m in zip(plan.elem_offsets, plan.numels):
        used[o:o + m] = True
    g = torch.Generator(device=DEV).manual_seed(7)
    base16 = torch.empty(n, device=DEV).normal_(0, 1, generator=g).bfloat16() if with_base else None
    base32, kept = (base16.float(), base16.clone()) if with_base else (None, None)
    sd = torch.arange(100, 100 + len(numels), dtype=torch.int32, device=DEV)
    ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
    planes = torch.empty(plan.planes_bytes, dtype=torch.uint8, device=DEV)
    scales = torch.empty(plan.n_slices, device=DEV)
    sums, y32, want = _nan(n, torch.float64), _nan(n, torch.float32), None
    for c, w in enumerate(W):
        plan.encode(torch.empty(n, device=DEV).normal_(0, 0.02, generator=g), sd, planes, scales, ws)
        plan.decode_accumulate(planes, sd, scales, sums, w, c == 0, None, ws, base=base16, bf16=True)
        plan.decode(planes, sd, scales, y32, ws, base=base32)
        want = y32.double() * w if c == 0 else want + y32.double() * w
    assert not want[used].isnan().any()
    assert torch.equal(sums.view(torch.int64)[used], want.view(torch.int64)[used])
    assert sums[~used].isnan().all()   # no gap and nothing past a length is touched
    assert not with_base or torch.equal(base16.view(torch.int16), kept.view(torch.int16))


@pytest.mark.parametrize("knobs", [{}, {"row2": 0}, {"pair": 1}], ids=["default", "row2_0", "pair_1"])
def test_row_launches_run_the_bf16_fold(knobs):
    from openfl_amd.codec import EdenPlan
    plan = EdenPlan(NUMELS, 8, **knobs)
    plain, bf = plan.accumulate_launches(), plan.accumulate_launches(bf16=True)
    row = "ofl::k_dec_acc_rowC" + ("" if "row2" in knobs else "2")
    assert len(plain) == len(bf)
    assert {(p["name"], b["name"]) for p, b in zip(plain, bf) if p["name"] != b["name"]} == {(row, row + "_bf16")}
    assert not any("k_dec_rowC" in b["name"] for b in bf)
    assert all(p["grid"] == b["grid"] and p["paired"] == b["paired"] for p, b in zip(plain, bf))


@functools.lru_cache(maxsize=None)
def _round():
    """The RoundEnd, three collaborators' uploads and a bf16 base, made once."""
    from openfl_amd.aggregation import RoundEnd
    from openfl_amd.pipelines import EdenPipeline
    pipe = EdenPipeline(n_bits=8, device=DEV, seed_mode="fast")
    re = RoundEnd(pipe, SHAPES, device=DEV)
    rng = np.random.default_rng(3)
    np.random.seed(5)
    uploads = [[pipe.forward((rng.standard_normal(s) * 0.02).astype(np.float32)) for s in SHAPES] for _ in W]
    return re, uploads, re.pack([rng.standard_normal(s) for s in SHAPES]).bfloat16()


def _stream_round(delta, base, out=None):
    re, uploads, _ = _round()
    acc = re.accumulator(sums=_nan(re.arena_numel, torch.float64))
    for items, w in zip(uploads, W):
        acc.add_upload(items, w, delta=delta, base_arena=base)
    sums = acc.sums.clone()
    np.random.seed(11)
    model, payloads, seeds = re.finish(acc, base_arena=base, out=out)
    return acc, sums, model, [(p, md_key(md)) for p, md in payloads], seeds


@pytest.mark.parametrize("delta", [True, False], ids=["delta", "full"])
def test_round_equals_the_float32_round_on_the_widened_base(delta):
    from openfl_amd._lib import CodecError
    re, uploads, base16 = _round()
    refused = re.accumulator()
    with pytest.raises(CodecError, match="bfloat16"):
        refused.add_upload(uploads[0], 1.0, delta=delta, base_arena=base16, fused=False)
    assert refused.weights == []
    acc32, sums32, model32, payloads32, seeds32 = _stream_round(delta, base16.float())
    acc16, sums16, model16, payloads16, seeds16 = _stream_round(delta, base16)
    assert acc16._scratch is None and acc32._scratch is not None
    assert not sums32.isnan().any() and torch.equal(sums16.view(torch.int64), sums32.view(torch.int64))
    assert payloads16 == payloads32 and seeds16 == seeds32
    assert model16.dtype == torch.bfloat16 and model32.dtype == torch.float32
    assert torch.equal(model16.view(torch.int16), model32.to(torch.bfloat16).view(torch.int16))
    assert (model16.view(torch.int16)[re._gap_idx] == 0).all()
    aliased = base16.clone()
    assert _stream_round(delta, aliased, out=aliased)[2] is aliased
    assert torch.equal(aliased.view(torch.int16), model16.view(torch.int16))
    for base, out in ((base16, model32), (base16.float(), model16)):
        acc = re.accumulator()
        acc.add(base16, 1.0)
        with pytest.raises(CodecError, match="base's dtype"):
            re.finish(acc, base_arena=base, out=out)


def test_add_takes_a_bf16_arena():
    re, _, _ = _round()
    g = torch.Generator(device=DEV).manual_seed(9)
    xs = [torch.empty(re.arena_numel, device=DEV).normal_(0, 1, generator=g).bfloat16() for _ in W]
    accs = [re.accumulator(sums=_nan(re.arena_numel, torch.float64)) for _ in range(2)]
    for x, w in zip(xs, W):
        accs[0].add(x, w)
        accs[1].add(x.float(), w)
    assert not accs[1].sums.isnan().any()
    assert torch.equal(accs[0].sums.view(torch.int64), accs[1].sums.view(torch.int64))
    assert torch.equal(accs[0]._table[:len(W)].view(torch.int32), accs[1]._table[:len(W)].view(torch.int32))
