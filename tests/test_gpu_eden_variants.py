"""GPU tests of the large-slice Eden path (slices above 2^15): every schedule
variant of tests/eden_variants.py bit-identical to the default plan, with the
launch list proving which kernels ran; and the edge inputs of the goldens
(all-zero, constant, one inf, overflowing, underflowing), generated at sizes
that reach the row / column kernels and k_finalize, against the CPU oracle.

Bars are those of tests/test_gpu_parity.py (imported, not restated)."""
import numpy as np
import pytest
import torch

from oracle import eden as O
from tests import eden_variants as V
from tests.test_gpu_parity import BIN_AGREE, DEV, _finite_scales_close, assert_decode_close, gpu_decode

pytestmark = pytest.mark.gpu


def _written(plan, planes, scales, y=None):
    """Views of the ranges a call writes (arena alignment gaps are never
    written): the scales, then every tensor's planes, then every tensor's y."""
    out = [scales[:plan.n_slices]]
    out += [planes[o:o + b] for o, b in zip(plan.planes_offsets, plan.planes_nbytes)]
    if y is not None:
        out += [y[o:o + n] for o, n in zip(plan.elem_offsets, plan.numels)]
    return out


def _assert_runs_what_it_says(cfg, plan):
    expl, paired = V.expected_shape(cfg)
    for enc in (True, False):
        L = plan.launches(enc)
        rows = [l for l in L if "_row" in l["name"]]
        assert any(l["expl"] for l in rows) == expl, (cfg, enc)
        assert any(l["paired"] for l in rows) == paired, (cfg, enc)
        assert all(l["paired"] <= ("_rowA2" in l["name"] if enc else "_rowC2" in l["name"]) for l in L), (cfg, enc)
        if expl:  # split: both 2^26 slices, every row launch of theirs over an explicit list
            assert all(l["expl"] and l["name"].split("<")[0].endswith("2") for l in rows), (cfg, enc)
            signs = [l for l in rows if ("_rowA2" in l["name"] if enc else "_rowC2" in l["name"])]
            assert all(l["paired"] == paired for l in signs), (cfg, enc)
        if cfg is not None and cfg[0] == 0:  # persistent kernels (encode pass C has none to choose)
            assert {l["name"].split("<")[0] for l in rows} == (
                {"ofl::k_enc_rowA", "ofl::k_enc_rowC2"} if enc else {"ofl::k_dec_rowA", "ofl::k_dec_rowC"}), (cfg, enc)
    if cfg is not None and cfg[2] == 64:
        assert plan.n_waves == 2, cfg  # a wave below the slice size, whether split or whole


def test_variants_bit_identical():
    """Every config of eden_variants.VARIANT_CONFIGS -- the default plan first
    -- over NUMELS: encode, decode and decode(base=...) give the default
    plan's planes, scales and values bit for bit over the written ranges
    (planes pre-filled with 0x5A, scales and outputs with NaN), and the launch
    list shows that the config ran what its name says: (-1, 0, 64) explicit
    tile lists and no pair, (0, -1, 64) whole-slice persistent passes at a
    wave below the slice, and so on.  decode_add has a real reference:
    y_add == base + y exactly, tensor by tensor (two fp32 roundings, decoded
    first, then the add: include/ofl_codec.h)."""
    g = torch.Generator(device=DEV)
    seeds = torch.tensor([5, 6, 7], dtype=torch.int32, device=DEV)
    ref = base = None
    for cfg in V.VARIANT_CONFIGS:
        plan = V.make_plan(cfg)
        _assert_runs_what_it_says(cfg, plan)
        if base is None:
            base = torch.empty(plan.arena_numel, device=DEV).normal_(0, 1.0, generator=g.manual_seed(22))
        x = torch.empty(plan.arena_numel, device=DEV).normal_(0, 0.01, generator=g.manual_seed(21))
        ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
        p = torch.full((plan.planes_bytes,), 0x5A, dtype=torch.uint8, device=DEV)
        s = torch.full((plan.n_slices,), float("nan"), dtype=torch.float32, device=DEV)
        plan.encode(x, seeds, p, s, ws)
        y = torch.full((plan.arena_numel,), float("nan"), dtype=torch.float32, device=DEV)
        plan.decode(p, seeds, s, y, ws)
        torch.cuda.synchronize()
        if ref is None:  # the default plan's round trip is Eden's (8 bits, Gaussian input)
            err = sum(float((y[o:o + n] - x[o:o + n]).double().square().sum())
                      for o, n in zip(plan.elem_offsets, plan.numels))
            tot = sum(float(x[o:o + n].double().square().sum()) for o, n in zip(plan.elem_offsets, plan.numels))
            assert 5.5e-3 < (err / tot) ** 0.5 < 7.5e-3, (err / tot) ** 0.5
        del x
        y2 = torch.full((plan.arena_numel,), float("nan"), dtype=torch.float32, device=DEV)
        plan.decode(p, seeds, s, y2, ws, base=base)
        torch.cuda.synchronize()
        del ws
        # the written ranges, tensor by tensor (views: nothing is copied)
        out = _written(plan, p, s, y)
        if ref is None:
            assert all(bool(torch.isfinite(t).all()) for t in out[1:])
            ref = [t.clone() for t in out]
        else:
            for k, (a, b) in enumerate(zip(out, ref)):
                assert torch.equal(a, b), (cfg, k)
        del out
        for t, (o, n) in enumerate(zip(plan.elem_offsets, plan.numels)):
            assert torch.equal(y2[o:o + n], base[o:o + n] + y[o:o + n]), (cfg, t)
        del p, s, y, y2
    del ref, base
    torch.cuda.empty_cache()


def test_row2_and_pair_rejected_after_first_encode():
    """The schedule (and its tile tables) is on the device after the first
    call: ofl_eden_plan_set_row2 / _set_pair then fail with OFL_EINVAL and
    leave the launch list as it was."""
    from openfl_amd import _lib
    from openfl_amd.codec import EdenPlan
    L = _lib.lib()
    plan = EdenPlan([1 << 16], 8)
    assert L.ofl_eden_plan_set_row2(plan.handle, 1) == _lib.OFL_OK
    before = (plan.launches(True), plan.launches(False))
    x = torch.zeros(plan.arena_numel, device=DEV)
    p = torch.zeros(plan.planes_bytes, dtype=torch.uint8, device=DEV)
    s = torch.zeros(plan.n_slices, dtype=torch.float32, device=DEV)
    ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
    plan.encode(x, torch.tensor([1], dtype=torch.int32, device=DEV), p, s, ws)
    torch.cuda.synchronize()
    for mode in (-1, 0, 1):
        assert L.ofl_eden_plan_set_row2(plan.handle, mode) == _lib.OFL_EINVAL
        assert b"row2" in L.ofl_last_error()
        assert L.ofl_eden_plan_set_pair(plan.handle, mode) == _lib.OFL_EINVAL
        assert b"pair" in L.ofl_last_error()
    assert (plan.launches(True), plan.launches(False)) == before


# ------------------------------------------------ edge inputs, large path ---
def _gen(n, seed, scale=0.01):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32) * np.float32(scale)


def edge_input(tag, n):
    """The goldens' edge recipes (tests/golden/make_golden.py) at size n; the
    inf sits at n - 17, so that only a tensor's last slice degenerates."""
    if tag == "zeros":
        return np.zeros(n, np.float32)
    if tag == "const":
        return np.full(n, 0.5, np.float32)
    if tag == "withinf":
        x = _gen(n, 7).copy()
        x[n - 17] = np.inf
        return x
    if tag == "huge":
        return _gen(n, 8) * np.float32(1e30)
    assert tag == "tiny"
    return _gen(n, 9) * np.float32(1e-30)


def _encode_over(x_dev, seeds, plan, fill=0xFF):
    """Encode into planes pre-filled with `fill` and NaN scales: stale bytes show."""
    planes = torch.full((max(plan.planes_bytes, 1),), fill, dtype=torch.uint8, device=DEV)
    scales = torch.full((max(plan.n_slices, 1),), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
    plan.encode(x_dev, torch.tensor(seeds, dtype=torch.int32, device=DEV), planes, scales, ws)
    torch.cuda.synchronize()
    return planes[:plan.planes_bytes], scales[:plan.n_slices]


# 65 536: one column level; 120 003: one ragged 2^17 slice; the third: dims
# [2^20, 2^17], only the second slice holds the inf; 2^23: two column levels
EDGE_SIZES = [65_536, 120_003, (1 << 20) + (1 << 16) + 5, 1 << 23]


@pytest.mark.parametrize("n", EDGE_SIZES)
@pytest.mark.parametrize("tag", ["zeros", "const", "withinf", "huge", "tiny"])
def test_edge_inputs_large_path_vs_oracle(tag, n):
    """Edge inputs on the row / column kernels and k_finalize, bits 2 and 8,
    seed 321, against oracle.eden.compress / decompress, encoded over a
    0xFF-filled buffer:
      * zeros, tiny (norm underflows to 0) and the slice holding the inf: the
        reference's zero fallback -- every plane byte 0, scale 0 (the `nu > 0`
        gate of encode pass C, the column pass's norm, k_finalize's zero-norm
        and NaN-scale branches);
      * huge (the norm overflows): planes and scales, infinities included,
        equal the oracle's;
      * const and the healthy first slice of the two-slice withinf: the bars
        of test_gpu_parity (>= 99.9 % of bins equal, |dbin| <= 1, scales
        within 1e-3);
      * our decoder on the oracle's bytes: assert_decode_close, or the
        oracle's isfinite pattern where its output is not finite.
    The 99.9 % bar counts rounding flips, so an input is admissible when the
    reference itself stays within half the bar of the oracle.  Reference vs
    oracle on the CPU, worst mismatching-bin fraction per size (2 / 8 bits):
      const    65 536: 0 / 0;  120 003: 0 / 0;  [2^20, 2^17]: 5.7e-6 / 3.4e-4;
               2^23: 1.1e-4 / 8.1e-3 (the reference's own fp32 norm of 2^23
               equal values is 7e-4 off the oracle's, scale 0.49968 vs
               0.50002: the reference is above the bar there before any GPU
               is involved; the kernels are held to the oracle all the same
               and measure 4.8e-7 / 8.1e-6 against it)
      withinf  first slice of [2^20, 2^17]: 3.8e-6 / 4.4e-4; every degenerate
               slice: 0
    `spike` (one nonzero element: discrete rotated values) gave 1.78e-3 at
    120 003 / 8 bits and is left out at these sizes."""
    from openfl_amd.codec import EdenPlan
    x = edge_input(tag, n)
    xd = torch.from_numpy(x).to(DEV)
    for bits in (2, 8):
        plan = EdenPlan([n], bits)
        dims = plan.dims[0]
        assert max(dims) > 1 << 15  # the large path
        gp, gs = _encode_over(xd, [321], plan)
        gp, gs = gp.cpu().numpy(), gs.cpu().numpy()
        op, osc, odims, _ = O.compress(x, 321, bits)
        assert dims == odims and gp.size == op.size
        P = sum(dims)
        if tag == "huge":
            assert np.array_equal(gp, op)
            assert np.array_equal(gs, np.asarray(osc, np.float32)) and not np.any(np.isfinite(gs))
        else:
            gb, ob = O.bins_of(gp, P, bits), O.bins_of(op, P, bits)
            rows = gp.reshape(bits, P // 8)
            off = 0
            for k, d in enumerate(dims):
                degenerate = tag in ("zeros", "tiny") or (tag == "withinf" and off <= n - 17 < off + d)
                a, b = gb[off:off + d], ob[off:off + d]
                print(f"[edge {tag} n={n} b={bits} slice {k}] mismatching bins {np.mean(a != b):.3e}, "
                      f"max |dbin| {np.max(np.abs(a - b))}, scale {gs[k]!r} vs {osc[k]!r}", flush=True)
                if degenerate:
                    assert not rows[:, off // 8:(off + d) // 8].any(), (bits, k)
                    assert gs[k] == 0.0 and osc[k] == 0.0 and not b.any(), (bits, k)
                else:
                    assert np.mean(a == b) >= BIN_AGREE, (bits, k, np.mean(a != b))
                    assert np.max(np.abs(a - b)) <= 1, (bits, k)
                off += d
            _finite_scales_close(gs, osc)
        y = gpu_decode(op, n, osc, odims, 321, bits)
        yo = O.decompress(op, n, osc, odims, 321, bits)
        if not np.all(np.isfinite(yo)):
            assert np.array_equal(np.isfinite(y), np.isfinite(yo))
        else:
            assert_decode_close(y, yo)


@pytest.mark.parametrize("tag", ["zeros", "withinf"])
def test_edge_inputs_five_pass_split(tag):
    """One 2^26 slice under the default plan -- the split schedule: four
    sub-wave launches store the slice's planes, then k_finalize finds a zero
    norm (zeros: nothing may have been stored but zeros) or a NaN scale
    (withinf: it rewrites every plane byte of the slice).  The expected
    output needs no oracle: all-zero planes, scale 0, and a decode of them
    that is exactly zero."""
    from openfl_amd.codec import EdenPlan
    n = 1 << 26
    plan = EdenPlan([n], 8)
    assert plan.dims == [[n]] and any(l["expl"] for l in plan.launches(True))
    if tag == "zeros":
        x = torch.zeros(n, device=DEV)
    else:
        x = torch.empty(n, device=DEV).normal_(0, 0.01, generator=torch.Generator(device=DEV).manual_seed(7))
        x[n - 17] = float("inf")
    planes, scales = _encode_over(x, [321], plan)
    assert int(torch.count_nonzero(planes)) == 0
    assert scales.cpu().tolist() == [0.0]
    y = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
    plan.decode(planes, torch.tensor([321], dtype=torch.int32, device=DEV), scales, y, ws)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(y)) == 0
    del x, y, ws, planes
    torch.cuda.empty_cache()


@pytest.mark.parametrize("wave_mib", [None, 0.5])
def test_edge_inputs_in_a_batch(wave_mib):
    """A zeros tensor and a withinf tensor between Gaussian ones, each >= 2^16,
    and a small one, in one two-stream plan -- with the default waves (one
    wave: every large slice in the same launches and one k_finalize) and with
    0.5 MiB waves alternating between the two streams (a k_finalize per
    stream): each tensor's planes and scales equal its own single-tensor
    encode, so a degenerate slice neither keeps stale bytes nor touches its
    neighbours."""
    from openfl_amd.codec import EdenPlan
    numels = [1 << 16, 65_536, 120_003, (1 << 18) + 5, 3000]
    xs = [_gen(numels[0], 1), edge_input("zeros", numels[1]), edge_input("withinf", numels[2]),
          _gen(numels[3], 2), _gen(numels[4], 3)]
    seeds = [11, 22, 33, 44, 55]
    plan = EdenPlan(numels, 8, wave_mib=wave_mib, streams=2)
    assert plan.n_streams == 2 and (plan.n_waves == 3 if wave_mib else plan.n_waves == 1)
    assert [l["name"] for l in plan.launches(True)].count("ofl::k_finalize") == (2 if wave_mib else 1)
    arena = torch.zeros(plan.arena_numel, device=DEV)
    for x, off in zip(xs, plan.elem_offsets):
        arena[off:off + x.size] = torch.from_numpy(x).to(DEV)
    planes, scales = _encode_over(arena, seeds, plan)
    planes, scales = planes.cpu().numpy(), scales.cpu().numpy()
    for t, (x, sd) in enumerate(zip(xs, seeds)):
        one = EdenPlan([x.size], 8)
        p1, s1 = _encode_over(torch.from_numpy(x).to(DEV), [sd], one)
        po, pb = plan.planes_offsets[t], plan.planes_nbytes[t]
        np.testing.assert_array_equal(planes[po:po + pb], p1.cpu().numpy(), err_msg=f"tensor {t}")
        fs = plan.first_slice[t]
        np.testing.assert_array_equal(scales[fs:fs + one.n_slices], s1.cpu().numpy(), err_msg=f"tensor {t}")
        if t in (1, 2):
            assert not p1.any() and not s1.any()
        else:
            assert bool(torch.isfinite(s1).all()) and bool((s1 > 0).all())
