"""Exact Eden encode checks on the GPU: designed inputs (tests/eden_exact.py)
whose bins and scales are known before the encoder runs, so the kernels are
held to every plane byte instead of to a 99.9 % agreement.

Bars, for every designed case (encode over 0xFF-filled planes and NaN scales):
  * plane bytes == expected_planes(designed bins), compared on the device;
  * |scale / alpha - 1| <= 2e-5.  Both sums behind a scale (|v|^2 and
    <C[bins], v>) add terms of one sign, so any summation order is within
    (longest chain of dependent adds) * 2^-24 of the exact sum, relatively.
    In these kernels a thread adds at most 64 terms, a 1024-thread block tree
    adds 10 levels, and k_finalize loops and trees over at most 16 384 tile
    partials: under 150 dependent adds for the numerator and the denominator
    each, 2 * 150 * 2^-24 = 1.8e-5 together (rotation noise, ~1e-7, included
    in the slack).  The observed worst value is printed;
  * the decoder on those planes with scale = alpha returns x within the
    suite's decode bars (assert_decode_close: relative L2 and max error
    2e-6; the oracle measures 3.2e-7), with plan.decode and, at 3 bits (one
    size of every class), also with decode_add onto a base: exactly
    base + decoded.
A mismatching plane byte is reported with element index, bin got / designed,
row tile (index >> 15) and lane (index & 63).

Ragged slices (len < P) cannot be designed: test_ragged_margin_rule holds
their bins to an fp64 rotation done on the device (eden_exact.margin_rule)
and their scale to the fp64 value |x|^2 / <C[gpu bins], v64> within 2e-5.

Observed on an MI355X, worst over the cases of a class (every plane byte
equal everywhere; |scale / alpha - 1| / round-trip relative L2 / round-trip
max error over max |x|; float32(0.01) itself is 2.2e-8 off 0.01):
  tiny and small kernels, [8] .. [1 << 15]    2.1e-7 / 1.6e-7 / 2.0e-7
  one column level, [1 << 16], [1 << 18]      2.1e-7 / 1.7e-7 / 2.1e-7
  multi-slice, [1 << 21, 8], [1 << 20, 1 << 17]  3.9e-7 / 1.8e-7 / 1.9e-7
  two column levels, [1 << 23], [1 << 25]     1.2e-7 / 2.0e-7 / 2.1e-7
  persistent rows, [1 << 18], 1..8 bits       2.1e-7 / 1.7e-7 / 2.1e-7
  five-pass, [1 << 26] (8 and 3 bits)         2.2e-8 / 2.0e-7 / 2.1e-7
  five-pass, [1 << 29]                        1.2e-7 / 2.1e-7 / 2.0e-7
  batch (both wave settings) 2.1e-7; wavg [1 << 16, 2048] 8.8e-8, [1 << 26] 2.2e-8
  ragged, share of elements inside tau / |scale / fp64 - 1|:
    8 bits  120 003: 3.6e-4 / 9.2e-8;  2^21 + 7: 4.9e-4 / 1.4e-7;  2^23 + 70 001: 5.5e-4 / 8.3e-8
    3 bits  120 003: 2.3e-5 / 3.9e-8;  2^21 + 7: 1.7e-5 / 1.4e-7;  2^23 + 70 001: 1.6e-5 / 1.0e-7
The slowest case, [1 << 29], takes 4.5 s; no other takes more than 0.8 s.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import eden as O
from tests import eden_exact as X
from tests.test_gpu_eden_variants import _encode_over
from tests.test_gpu_parity import DEV, assert_decode_close

pytestmark = pytest.mark.gpu

SCALE_BAR = 2e-5
DECODE_BAR = 2e-6          # assert_decode_close's, restated for the on-device form
HOST_COMPARE_MAX = 1 << 23


def _assert_planes_exact(got, want, bins, bits, what):
    if torch.equal(got, want):
        return
    Ptot = bins.numel()
    gb = X.bins_from_planes(got.contiguous(), Ptot, bits)
    bad = torch.nonzero(gb != bins).reshape(-1)
    head = [(int(i), int(gb[i]), int(bins[i]), int(i) >> 15, int(i) & 63) for i in bad[:16]]
    raise AssertionError(f"{what}: {bad.numel()} of {Ptot} bins differ from the designed ones; "
                         f"(index, got, designed, tile, lane): {head}")


def _assert_decode_close(y, x):
    """assert_decode_close; above HOST_COMPARE_MAX elements the same two bars
    in fp64 on the device.  -> (relative L2, max err / max |x|)."""
    e = (y.double() - x.double())
    rel = float(torch.linalg.vector_norm(e) / torch.linalg.vector_norm(x.double()))
    mx = float(e.abs().max() / x.abs().max())
    del e
    if x.numel() <= HOST_COMPARE_MAX:
        assert_decode_close(y.cpu().numpy(), x.cpu().numpy())
    else:
        assert rel <= DECODE_BAR and mx <= DECODE_BAR, (rel, mx)
    return rel, mx


def _check_designed(plan, dims, bits, x, bins, alphas, what, decode_add=False):
    """One designed tensor alone in `plan`: planes, scales and the decode."""
    assert plan.dims == [dims] and plan.elem_offsets == [0]
    want = X.expected_planes(bins, dims, bits)
    planes, scales = _encode_over(x, [X.SEED], plan)
    assert planes.numel() == want.numel()
    _assert_planes_exact(planes, want, bins, bits, what)
    a = torch.tensor(alphas, dtype=torch.float64, device=DEV)
    worst = float((scales.double() / a - 1).abs().max())
    # decode of the designed planes with scale = alpha
    sd = torch.tensor([X.SEED], dtype=torch.int32, device=DEV)
    ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
    y = torch.full((plan.arena_numel,), float("nan"), dtype=torch.float32, device=DEV)
    plan.decode(want, sd, a.float(), y, ws)
    torch.cuda.synchronize()
    rel, mx = _assert_decode_close(y, x)
    print(f"[designed {what} b={bits}] |scale/alpha-1| {worst:.2e}  round trip rel L2 {rel:.2e} max {mx:.2e}",
          flush=True)
    assert worst <= SCALE_BAR, (what, scales.tolist(), alphas)
    if decode_add:
        base = torch.empty_like(x).normal_(0, 1.0, generator=torch.Generator(device=DEV).manual_seed(22))
        y2 = torch.full_like(y, float("nan"))
        plan.decode(want, sd, a.float(), y2, ws, base=base)
        torch.cuda.synchronize()
        assert torch.equal(y2, base + y), what
        del base, y2
    del y, ws, planes, want


SMALL = [[8], [64], [1024], [2048], [1 << 15], [1 << 16], [1 << 18]]
LARGE = [[1 << 21, 8], [1 << 20, 1 << 17], [1 << 23], [1 << 25]]
CASES = [(d, b) for d in SMALL for b in range(1, 9)] + [(d, b) for d in LARGE for b in (1, 3, 8)]


@pytest.mark.parametrize("dims,bits", CASES, ids=lambda v: "_".join(map(str, v)) if isinstance(v, list) else f"b{v}")
def test_designed_exact(dims, bits):
    """Default plans.  [8] .. [2048]: tiny and small kernels; up to [1 << 15]
    the small-set launch; [1 << 16]: one column level; [1 << 18]: slices that
    may pair; [1 << 21, 8]: odd-length plane rows (the byte-wise plane
    paths); [1 << 20, 1 << 17]: two slices with different alpha; [1 << 23]:
    two column levels; [1 << 25]: the interleaved layout."""
    from openfl_amd.codec import EdenPlan
    x, bins, alphas = X.designed(dims, bits, device=DEV)
    plan = EdenPlan([sum(dims)], bits)
    _check_designed(plan, dims, bits, x, bins, alphas, str(dims), decode_add=bits == 3)


@pytest.mark.parametrize("bits", range(1, 9))
def test_designed_exact_persistent_rows(bits):
    """k_enc_rowA, k_dec_rowA and k_dec_rowC (row2 = 0: the auto rule never
    picks them below five tiles per CU, so no other test runs them at a width
    other than 8), one 2^18 slice, every width."""
    from openfl_amd.codec import EdenPlan
    dims = [1 << 18]
    plan = EdenPlan(dims, bits, wave_mib=4096, streams=1, row2=0, pair=0)
    for enc, names in ((True, {"ofl::k_enc_rowA", "ofl::k_enc_rowC2"}), (False, {"ofl::k_dec_rowA", "ofl::k_dec_rowC"})):
        rows = {l["name"].split("<")[0] for l in plan.launches(enc) if "_row" in l["name"]}
        assert rows == names, rows
    x, bins, alphas = X.designed(dims, bits, device=DEV)
    _check_designed(plan, dims, bits, x, bins, alphas, "persistent rows [1 << 18]", decode_add=True)


@pytest.mark.parametrize("p,bits", [(26, 8), (26, 3), (29, 8)])
def test_designed_exact_five_pass(p, bits):
    """One five-pass slice under the default plan (split into sub-waves,
    paired): 2^26, and 2^29, the Llama-3-8B embedding's slice -- the exact
    encode check at that size.  x, the expected planes and every comparison
    stay on the device."""
    from openfl_amd.codec import EdenPlan
    dims = [1 << p]
    plan = EdenPlan(dims, bits)
    rows = [l for l in plan.launches(True) if "_row" in l["name"]]
    assert any(l["expl"] for l in rows) and any(l["paired"] for l in rows)
    x, bins, alphas = X.designed(dims, bits, device=DEV)
    _check_designed(plan, dims, bits, x, bins, alphas, f"five-pass [1 << {p}]", decode_add=bits == 3)
    del x, bins
    torch.cuda.empty_cache()


@pytest.mark.parametrize("wave_mib", [None, 0.5])
def test_designed_batch_exact(wave_mib):
    """Five designed tensors, each with its own seed and alphas, in one plan,
    with the default waves and with 0.5 MiB waves: every tensor's planes and
    scales are exact inside the batch."""
    from openfl_amd.codec import EdenPlan
    bits = 8
    all_dims = [[1 << 16], [2048], [1 << 18], [1 << 20, 1 << 17], [64]]
    seeds = [11, 22, 33, 44, 55]
    plan = EdenPlan([sum(d) for d in all_dims], bits, wave_mib=wave_mib)
    assert plan.dims == all_dims and (plan.n_waves > 1 if wave_mib else plan.n_waves == 1)
    arena = torch.zeros(plan.arena_numel, device=DEV)
    want = []
    for t, (dims, sd) in enumerate(zip(all_dims, seeds)):
        alphas = [0.01 * (t + 1) * (1 + 2 * k) for k in range(len(dims))]
        x, bins, _ = X.designed(dims, bits, seed=sd, alphas=alphas, device=DEV)
        arena[plan.elem_offsets[t]:plan.elem_offsets[t] + x.numel()] = x
        want.append((bins, alphas))
    planes, scales = _encode_over(arena, seeds, plan)
    worst = 0.0
    for t, (dims, (bins, alphas)) in enumerate(zip(all_dims, want)):
        po, pb = plan.planes_offsets[t], plan.planes_nbytes[t]
        _assert_planes_exact(planes[po:po + pb], X.expected_planes(bins, dims, bits), bins, bits, f"tensor {t}")
        fs = plan.first_slice[t]
        a = torch.tensor(alphas, dtype=torch.float64, device=DEV)
        worst = max(worst, float((scales[fs:fs + len(dims)].double() / a - 1).abs().max()))
    print(f"[designed batch wave_mib={wave_mib}] |scale/alpha-1| {worst:.2e}", flush=True)
    assert worst <= SCALE_BAR


@pytest.mark.parametrize("dims", [[1 << 16, 2048], [1 << 26]], ids=lambda d: "_".join(map(str, d)))
def test_designed_wavg_exact(dims):
    """ofl_eden_encode_wavg, the fused round-end encode, against something
    other than the HIP encode: two collaborator arenas that both hold the
    designed x, weights 0.5 / 0.5, no base, the delta arena = x -- the average
    is x exactly (x/2 + x/2 in fp64), so planes and scales are the designed
    ones.  [1 << 26] is the split path, its pass A unpaired."""
    from openfl_amd import _lib
    from openfl_amd.codec import EdenPlan
    bits = 8
    x, bins, alphas = X.designed(dims, bits, device=DEV)
    plan = EdenPlan([sum(dims)], bits)
    assert plan.dims == [dims]
    if dims == [1 << 26]:
        assert any(l["expl"] for l in plan.launches(True))
    xs = [x, x.clone()]
    ptrs = torch.tensor([t.data_ptr() for t in xs], dtype=torch.int64, device=DEV)
    w = torch.tensor([0.5, 0.5], dtype=torch.float64, device=DEV)
    seeds = torch.tensor([X.SEED], dtype=torch.int32, device=DEV)
    ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
    p = torch.full((plan.planes_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
    s = torch.full((plan.n_slices,), float("nan"), dtype=torch.float32, device=DEV)
    delta = x.clone()
    _lib.check(_lib.lib().ofl_eden_encode_wavg(plan.handle, ptrs.data_ptr(), w.data_ptr(), 2, ctypes.c_double(1.0),
                                               None, delta.data_ptr(), seeds.data_ptr(), p.data_ptr(),
                                               s.data_ptr(), ws.data_ptr(), ws.numel(), None))
    torch.cuda.synchronize()
    _assert_planes_exact(p, X.expected_planes(bins, dims, bits), bins, bits, f"wavg {dims}")
    worst = float((s.double() / torch.tensor(alphas, dtype=torch.float64, device=DEV) - 1).abs().max())
    print(f"[designed wavg {dims}] |scale/alpha-1| {worst:.2e}", flush=True)
    assert worst <= SCALE_BAR
    del xs, delta, p, ws, x, bins
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", [120_003, (1 << 21) + 7, (1 << 23) + 70_001])
@pytest.mark.parametrize("bits", [8, 3])
def test_ragged_margin_rule(n, bits):
    """Gaussian input N(0, 0.01^2) on slices with a ragged tail: every bin
    farther than tau from all boundaries equals the fp64 bin, a nearer one
    lies on one side or the other of that boundary (eden_exact.margin_rule,
    tau = 4 x the oracle's own fp32 rotation error on this input); at most
    1e-3 of the elements are that near; every scale is within 2e-5 of
    |x|^2 / <C[gpu bins], v64>."""
    from openfl_amd.codec import EdenPlan
    x = torch.from_numpy(np.random.default_rng(n + bits).standard_normal(n).astype(np.float32)
                         * np.float32(0.01)).to(DEV)
    plan = EdenPlan([n], bits)
    dims = plan.dims[0]
    Ps, Ls = O.slice_plan(n)
    assert dims == Ps and any(l < P for l, P in zip(Ls, Ps))
    planes, scales = _encode_over(x, [X.SEED], plan)
    got = X.bins_from_planes(planes, sum(dims), bits)
    v64 = X.rotated64(x, n, dims, X.SEED)
    share = X.margin_rule(x, n, dims, bits, X.SEED, got, v64=v64)
    C = torch.from_numpy(O.tables(bits)[0].astype(np.float64)).to(DEV)
    off = src = 0
    worst = 0.0
    for k, (P, ln, v) in enumerate(zip(Ps, Ls, v64)):
        ref = float(x[src:src + ln].double().square().sum() / torch.dot(C[got[off:off + P].long()], v))
        worst = max(worst, abs(float(scales[k]) / ref - 1))
        off += P
        src += ln
    print(f"[ragged n={n} b={bits}] share inside tau {share:.2e}  |scale/fp64-1| {worst:.2e}", flush=True)
    assert share <= 1e-3, share
    assert worst <= SCALE_BAR, worst
