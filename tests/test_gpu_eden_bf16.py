"""Eden encode from and decode into bfloat16 arenas (EdenPlan.encode / decode
with torch.bfloat16, ofl_eden_encode_bf16 / ofl_eden_decode_add_bf16,
csrc/eden_bf16.h), held to the float32 path of the same library, which the
other GPU tests hold to the oracle, and to torch's own .to(torch.bfloat16).
Everything is bit for bit (int16 / uint8 / int32 views): widening bf16 is
exact, and decode adds one defined rounding.

NUMELS by the reference's slicing rule: 60001 one 2^16 slice (two tiles, the
last quad holds 1 valid element); 125003 one 2^17 slice (a tail of 3); 480001
one 2^19 slice (tile 14 partial with a tail of 1, tile 15 without a valid
element; its tiles pair up under pair=1); 98311 slices 2^16 + 2^15 + 8 (large,
small and tiny in one tensor); 4099 and 101 small; 7 tiny.  The default plan
runs the two-blocks-per-CU variants unpaired; row2=0 the persistent ones,
pair=1 the paired table, and one 2^26 slice at 64 MiB waves the explicit,
paired tile lists of its sub-waves."""
import numpy as np
import pytest
import torch

from oracle import eden as O
from tests import eden_walsh as W
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

NUMELS = [60001, 125003, 480001, 98311, 4099, 101, 7]
SEEDS = [[100, 101, 102, 103, 104, 105, 106], [65535, 0, 321, 7, 40000, 9, 12345]]
SPLIT = {"wave_mib": 64, "streams": 1}
CASES = [(NUMELS, b, s, {}) for b in (1, 4, 8) for s in SEEDS] + \
        [(NUMELS, 8, SEEDS[0], {"row2": 0}), (NUMELS, 4, SEEDS[1], {"pair": 1}), ([1 << 26], 8, [77], SPLIT)]
IDS = [f"{len(n)}t-{b}b-s{s[0]}-{'_'.join(f'{k}{v}' for k, v in kw.items()) or 'default'}" for n, b, s, kw in CASES]
SENTINEL = 0x5A5A


def _sentinel(n):
    return torch.full((n,), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _i16(t):
    return t.view(torch.int16)


def _used(plan):
    used = torch.zeros(plan.arena_numel, dtype=torch.bool, device=DEV)
    for o, n in zip(plan.elem_offsets, plan.numels):
        used[o:o + n] = True
    return used


@pytest.mark.parametrize("numels,bits,seeds,knobs", CASES, ids=IDS)
def test_bf16_arenas_equal_the_float32_path(numels, bits, seeds, knobs):
    from openfl_amd.codec import EdenPlan, slice_plan
    plan = EdenPlan(numels, bits, **knobs)
    n, used = plan.arena_numel, _used(plan)
    small = sum(ln for m in numels for P, ln in zip(*slice_plan(m)) if P <= 1 << 15)
    assert small <= plan.side_numel <= small + 6 * len(numels) and (small or not plan.side_numel)   # not an arena
    g = torch.Generator(device=DEV).manual_seed(5)
    x16 = torch.empty(n, device=DEV).normal_(0, 0.01, generator=g).bfloat16()
    base16 = torch.empty(n, device=DEV).normal_(0, 0.1, generator=g).bfloat16()
    sd = torch.tensor(seeds, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
    out = {}
    for x in (x16.float(), x16):
        planes = torch.full((plan.planes_bytes,), 0xA5, dtype=torch.uint8, device=DEV)
        scales = torch.full((plan.n_slices,), float("nan"), device=DEV)
        plan.encode(x, sd, planes, scales, ws)
        out[x.dtype] = planes, scales
    planes, scales = out[torch.float32]
    assert torch.equal(out[torch.bfloat16][0], planes)
    assert torch.equal(out[torch.bfloat16][1].view(torch.int32), scales.view(torch.int32))
    for base in (None, base16):
        y32 = torch.full((n,), float("nan"), device=DEV)
        plan.decode(planes, sd, scales, y32, ws, base=None if base is None else base.float())
        y16 = _sentinel(n)
        plan.decode(planes, sd, scales, y16, ws, base=base)
        assert not y32[used].isnan().any()
        assert torch.equal(_i16(y16)[used], _i16(y32.to(torch.bfloat16))[used])
        assert (_i16(y16)[~used] == SENTINEL).all()
    ya = base16.clone()
    plan.decode(planes, sd, scales, ya, ws, base=ya)   # y_arena aliasing base
    assert torch.equal(_i16(ya)[used], _i16(y16)[used]) and torch.equal(_i16(ya)[~used], _i16(base16)[~used])


@pytest.mark.parametrize("numels,knobs,enc,dec", [
    (NUMELS, {}, "k_enc_rowA2_bf16", "k_dec_rowC2_bf16"), (NUMELS, {"row2": 0}, "k_enc_rowA_bf16", "k_dec_rowC_bf16"),
    (NUMELS, {"pair": 1}, "k_enc_rowA2_bf16", "k_dec_rowC2_bf16"), ([1 << 26], SPLIT, "k_enc_rowA2_bf16", "k_dec_rowC2_bf16")],
    ids=["default", "row2_0", "pair_1", "split"])
def test_row_launches_run_the_bf16_variants(numels, knobs, enc, dec):
    from openfl_amd.codec import EdenPlan
    plan = EdenPlan(numels, 8, **knobs)
    for d, want in ((True, enc), (False, dec)):
        plain, bf = plan.launches(d), plan.bf16_launches(d)
        swapped = [(p["name"], b["name"]) for p, b in zip(plain, bf) if p["name"] != b["name"]]
        assert swapped and set(swapped) == {("ofl::" + want[:-5], "ofl::" + want)}
        rows = [b for b in bf if b["name"] == "ofl::" + want]
        assert any(r["paired"] for r in rows) == ("pair" in knobs or knobs is SPLIT)
        assert all(r["expl"] for r in rows) == (knobs is SPLIT)
        assert all(2 * b["bytes_alg"] == p["bytes_alg"] for p, b in zip(plain, bf) if p["name"] != b["name"])


# float32 words whose rounding to bf16 is designed: ties with an even and an
# odd kept mantissa, just below and just above a tie, the carry into the
# exponent, the largest finite value (-> inf)
WORDS = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3FFFFFFF, 0x7F7FFFFF]
# and scales whose products are +-0, a float32 denormal, +-inf and NaN
SPECIAL = [0.0, 5e-39, float("inf"), float("nan")]


def _walsh_run(bits, word):
    """(k, j, scale) of a Walsh slice whose every output is +-the float32 word:
    fl32(scale * C[k]) == word for a float32 neighbour of word / C[k]."""
    C = O.tables(bits)[0]
    t = np.array([word], np.uint32).view(np.float32)[0]
    for k in range(1 << (bits - 1), 1 << bits):
        with np.errstate(over="ignore"):
            s = np.float32(t / C[k])
        for c in (s, np.nextafter(s, np.float32(0)), np.nextafter(s, np.float32(np.inf))):
            if np.isfinite(c) and int(W.product_bits(bits, k, c)) == word:
                return k, 5, float(c)
    raise AssertionError(f"no centroid and scale give {word:#x}")


def test_narrow_rounds_designed_values_as_torch_does():
    """A plan of small slices only: the narrow range kernel does every
    rounding.  The side arena's values are designed through the decode's own
    inputs (Walsh planes, tests/eden_walsh.py: every output of slice t is
    +-fl32(scale_t * C[k_t]), exactly)."""
    from openfl_amd.codec import EdenPlan
    bits = 8
    runs = [_walsh_run(bits, w) for w in WORDS] + [(200, 5, s) for s in SPECIAL]
    plan = EdenPlan([2048] * len(runs), bits)
    planes, scales, sd, want, valid = W.build_batch(plan, [(40 + t, [r]) for t, r in enumerate(runs)], bits, DEV)
    for o, w in zip(plan.elem_offsets, WORDS):
        assert ((want[o:o + 2048] & 0x7FFFFFFF) == w).all()
    assert valid.all() and not any("_row" in l["name"] for l in plan.bf16_launches(False))
    ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
    y16 = _sentinel(plan.arena_numel)
    plan.decode(planes, sd, scales, y16, ws)
    ref = want.cpu().view(torch.float32).to(torch.bfloat16)
    got = y16.cpu()
    nan = ref.isnan()
    assert nan.sum() == 2048 and torch.equal(got.isnan(), nan)
    assert torch.equal(_i16(got)[~nan], _i16(ref)[~nan])
    assert {0x0000, 0x8000 - (1 << 16), 0x7F80, 0xFF80 - (1 << 16), 0x4000} <= set(_i16(got).unique().tolist())


@pytest.mark.parametrize("case", ["mixed", "float16", "roundtrip", "short"])
def test_refused_arenas_launch_nothing(case):
    from openfl_amd._lib import CodecError
    from openfl_amd.codec import EdenPlan
    plan = EdenPlan([1 << 16, 1000], 8)
    n = plan.arena_numel
    sd = torch.tensor([1, 2], dtype=torch.int32, device=DEV)
    ws = torch.empty(max(plan.ws_bytes, plan.roundtrip_ws_bytes), dtype=torch.uint8, device=DEV)
    planes = torch.full((plan.planes_bytes,), 0xA5, dtype=torch.uint8, device=DEV)
    scales = torch.full((plan.n_slices,), float("nan"), device=DEV)
    plan.encode(torch.zeros(n, device=DEV), sd, planes, scales, ws)
    y16, y32 = _sentinel(n), torch.full((n,), float("nan"), device=DEV)
    planes2, scales2 = torch.full_like(planes, 0xA5), torch.full_like(scales, float("nan"))
    with pytest.raises(CodecError):
        if case == "mixed":
            plan.decode(planes, sd, scales, y16, ws, base=torch.zeros(n, device=DEV))
        elif case == "float16":
            plan.encode(torch.zeros(n, device=DEV).half(), sd, planes2, scales2, ws)
        elif case == "roundtrip":
            plan.roundtrip(torch.zeros(n, device=DEV).bfloat16(), sd, y32, scales2, ws)
        else:
            plan.decode(planes, sd, scales, y16[:n - 1], ws)
    if case == "mixed":   # and the other way round
        with pytest.raises(CodecError):
            plan.decode(planes, sd, scales, y32, ws, base=torch.zeros(n, device=DEV).bfloat16())
    if case == "float16":
        with pytest.raises(CodecError):
            plan.decode(planes, sd, scales, y32.half(), ws)
    torch.cuda.synchronize()
    assert (_i16(y16) == SENTINEL).all() and y32.isnan().all()
    assert (planes2 == 0xA5).all() and scales2.isnan().all()
