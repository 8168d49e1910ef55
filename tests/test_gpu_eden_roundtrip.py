"""The Eden round trip (EdenPlan.roundtrip, k_rt_row): y = decode(encode(x))
without planes.

1. Designed inputs (tests/eden_exact.py): the scales are alpha within
   SCALE_BAR (test_gpu_eden_exact.py's derivation: the partial sums are the
   encode's) and y is x within SCALE_BAR + DECODE_BAR, relative L2 and max
   error over max |x| in fp64 on the device -- the round trip multiplies by
   its own scale, not by alpha.
2. The specification: y and the scales are torch.equal to plan.decode(
   plan.encode(x)), with a base and with y aliasing the base too.
3. The launch list has k_rt_row and neither k_enc_rowC2 nor k_dec_rowA2.
4. RoundEnd.run(payloads=False) leaves run(payloads=True)'s model.

Observed on an MI355X, worst over the designed cases ([1 << 20, 1 << 17] at
3 bits): |scale / alpha - 1| 3.9e-7, relative L2 3.6e-7, max error over
max |x| 4.6e-7; elsewhere at most 1.2e-7 / 2.3e-7 / 2.8e-7.  The file takes
4.5 s.
"""
import numpy as np
import pytest
import torch

from tests import eden_exact as X
from tests.test_gpu_eden_exact import DECODE_BAR, SCALE_BAR
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

DIMS = [[1 << 16], [1 << 18], [1 << 21, 8], [1 << 20, 1 << 17], [1 << 23], [1 << 25], [1 << 26]]
CASES = [(d, b) for d in DIMS for b in (8, 3)] + [([1 << 16], 1)]
BATCH = [5, 1000, 4096, 70_000, 1 << 20, 3]
IDS = lambda v: "_".join(map(str, v)) if isinstance(v, list) else str(v)  # noqa: E731


def _roundtrip(plan, x, sd, base=None, out=None):
    y = torch.full((plan.arena_numel,), float("nan"), dtype=torch.float32, device=DEV) if out is None else out
    scales = torch.full((plan.n_slices,), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(max(plan.roundtrip_ws_bytes, 256), dtype=torch.uint8, device=DEV)
    plan.roundtrip(x, sd, y, scales, ws, base=base)
    torch.cuda.synchronize()
    return y, scales


@pytest.mark.parametrize("dims,bits", CASES, ids=IDS)
def test_designed_ground_truth(dims, bits):
    from openfl_amd.codec import EdenPlan
    x, _, alphas = X.designed(dims, bits, device=DEV)
    plan = EdenPlan([sum(dims)], bits)
    assert plan.dims == [dims]
    y, scales = _roundtrip(plan, x, torch.tensor([X.SEED], dtype=torch.int32, device=DEV))
    worst = float((scales.double() / torch.tensor(alphas, dtype=torch.float64, device=DEV) - 1).abs().max())
    e = y.double() - x.double()
    rel = float(torch.linalg.vector_norm(e) / torch.linalg.vector_norm(x.double()))
    mx = float(e.abs().max() / x.abs().max())
    print(f"[roundtrip designed {dims} b={bits}] |scale/alpha-1| {worst:.2e}  rel L2 {rel:.2e} max {mx:.2e}", flush=True)
    assert worst <= SCALE_BAR, (scales.tolist(), alphas)
    assert rel <= SCALE_BAR + DECODE_BAR and mx <= SCALE_BAR + DECODE_BAR, (rel, mx)


SPEC = [([sum(d)], b, None) for d, b in CASES] + [([120_003], 8, None), ([(1 << 23) + 70_001], 8, None),
                                                  (BATCH, 8, None), (BATCH, 8, 0.5)]


@pytest.mark.parametrize("numels,bits,wave_mib", SPEC, ids=IDS)
def test_is_decode_of_encode(numels, bits, wave_mib):
    from openfl_amd.codec import EdenPlan
    plan = EdenPlan(numels, bits, wave_mib=wave_mib)
    assert wave_mib is None or plan.n_waves > 1
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.empty(plan.arena_numel, device=DEV).normal_(0, 0.02, generator=g)
    base = torch.empty(plan.arena_numel, device=DEV).normal_(0, 1.0, generator=g)
    sd = torch.arange(100, 100 + len(numels), dtype=torch.int32, device=DEV)
    planes = torch.empty(max(plan.planes_bytes, 1), dtype=torch.uint8, device=DEV)
    want_s = torch.empty(plan.n_slices, device=DEV)
    ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
    plan.encode(x, sd, planes, want_s, ws)
    want, want_b = (torch.full_like(x, float("nan")) for _ in range(2))
    plan.decode(planes, sd, want_s, want, ws)
    plan.decode(planes, sd, want_s, want_b, ws, base=base)
    y, scales = _roundtrip(plan, x, sd)
    assert torch.equal(scales, want_s)
    yb = _roundtrip(plan, x, sd, base=base)[0]
    alias = base.clone()
    _roundtrip(plan, x, sd, base=alias, out=alias)
    for o, n in zip(plan.elem_offsets, numels):  # the tensors: the alignment gaps are not written
        assert torch.equal(y[o:o + n], want[o:o + n]) and not want[o:o + n].isnan().any()
        assert torch.equal(yb[o:o + n], want_b[o:o + n])
        assert torch.equal(alias[o:o + n], want_b[o:o + n])


@pytest.mark.parametrize("p", [23, 26])
def test_launch_list(p):
    from openfl_amd.codec import EdenPlan
    L = EdenPlan([1 << p], 8).roundtrip_launches()
    names = [l["name"] for l in L]
    assert "ofl::k_rt_row" in names and "ofl::k_enc_rowC2" not in names and "ofl::k_dec_rowA2" not in names
    assert (p != 26) or any(l["expl"] for l in L if l["name"] == "ofl::k_rt_row")


@pytest.mark.parametrize("kw", [{"fused": True}, {"fused": False}, {"aggregation": "median"}], ids=str)
def test_round_end_without_payloads(kw):
    from openfl_amd.aggregation import RoundEnd
    from openfl_amd.pipelines.eden_pipeline import EdenPipeline
    shapes = [(300,), (70_000,), (1 << 16,), (50,)]
    rng = np.random.default_rng(3)
    collabs = [[rng.standard_normal(s).astype(np.float32) for s in shapes] for _ in range(3)]
    base = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    re = RoundEnd(EdenPipeline(n_bits=8, device=DEV, seed_mode="fast"), shapes, DEV, **kw)
    arenas, base_a = [re.pack(c) for c in collabs], re.pack(base)
    w = None if "aggregation" in kw else [0.2, 0.3, 0.5]
    outs = []
    for payloads in (True, False):
        np.random.seed(11)
        outs.append(re.run(arenas, w, base_a, payloads=payloads)[0])
    for i in range(len(shapes)):
        assert torch.equal(re.view(outs[0], i), re.view(outs[1], i)), i
