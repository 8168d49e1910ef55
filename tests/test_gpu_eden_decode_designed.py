"""Exact Eden decode checks on the GPU: planes whose decode is known bit for
bit before the decoder runs (tests/eden_walsh.py), planes no encoder writes,
scales no encoder writes, and planes pointers of every alignment.

1. Walsh planes (bins k / 2^b - 1 - k in the pattern of Hadamard row j):
   every output word equals fl32(scale * C[k]) with the sign d2[j] h_j[e]
   d1[e], in every kernel class, with plan.decode and with base= (exactly
   base + expected in float32).  Outputs go into NaN-filled arenas and are
   compared on the device as int32 words; the words no decode may write
   (arena gaps, the padding of a ragged slice, 64 elements past the end) must
   keep the fill.  A mismatch reports element index, got / want, row tile
   (index >> 15) and lane (index & 63).
   Limits: a run uses two bin values (k and its mirror), D2 is probed at
   index j only (D1 at every element).  Parts 1 (every k of the lower half,
   many j, per width) and 3 (all bins in every lane) cover them.
2. Ragged outputs (the valid length ends inside a float4; one row tile has no
   valid output) and five tensors of different classes in one plan.
3. Foreign planes (uniform bytes; a sea of the two central bins with 64
   extreme ones; 0x00 and 0xFF, which are Walsh j = 0 and compared exactly)
   against eden_exact.unrotate in float64 on the device.  Bar per case:
   relative L2 and max error (over max |ref|) <= 4 x the C oracle's own fp32
   error against the same fp64 decode of the same planes (the factor is
   eden_exact.margin_rule's: another butterfly order).
   At [1 << 26] one element of a Gaussian-bin plane set is moved by one bin:
   the new bar refuses it by a factor above 2.  The suite's 2e-6 bars
   (assert_decode_close) sit 4 % below the fault at this size, in relative L2
   and in max error alike (delta / sqrt(P) = 2.06e-6 for the smallest
   centroid gap of the 8-bit table, 0.01689), and no longer see it from 2^27
   on (1.46e-6; 7.3e-7 at 2^29).
4. Scales from the wire: -0.0123, 0.0, -0.0, 1e-42, FLT_MAX, +inf, NaN; the
   expectation is the float32 product in NumPy (the oracle's arithmetic: it
   multiplies by the scale last), compared as bits, NaN-ness for NaN.
5. A planes pointer 1, 3, 4 and 7 bytes into its allocation: decode equals
   the aligned call and the expectation; encode writes the aligned call's
   bytes and nothing before or after its range; ofl_eden_encode_wavg
   likewise against its own aligned call.

Observed on an MI355X.  Parts 1, 2, 4 and 5 and the 0x00 / 0xFF planes: every
word equal in every case (before fold_scale, scale 1e-42 gave +-0 for
+-4.6e-42 at [1 << 16] and [1 << 23]; [64] and [2048] were equal).  Part 3,
worst over uniform / sea and 8 / 3 bits of a class, relative L2 / max error
over max |ref|, kernels then oracle, each against the fp64 decode:
  [2048]         1.36e-7 / 2.50e-7    oracle 1.62e-7 / 1.87e-7
  [1 << 16]      1.54e-7 / 2.00e-7    oracle 1.85e-7 / 2.13e-7
  [1 << 21, 8]   1.77e-7 / 1.72e-7    oracle 2.18e-7 / 2.14e-7
  [1 << 23]      1.86e-7 / 2.11e-7    oracle 2.27e-7 / 2.43e-7
  [1 << 26]      1.97e-7 / 2.09e-7    oracle 2.35e-7 / 2.59e-7
  (the nearest case to its bar: sea [2048] 8 bits, max error 2.50e-7 against
  4 x 1.87e-7)
One moved bin at [1 << 26]: unmoved planes 1.97e-7 / 1.85e-7, moved planes
2.07e-6 / 2.08e-6, oracle 2.35e-7 / 2.25e-7 (the bar: 9.4e-7 / 9.0e-7).
Time: the 125 cases take 9.4 s together; the slowest is
test_walsh_small_classes[8] (8704 tensors in the first of its three plans)
at 1.0 s, then [1 << 26] at 8 bits (Walsh and uniform planes) at 0.7 s each.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import eden as O
from tests import eden_exact as X
from tests import eden_walsh as W
from tests.test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

PAD = 64            # elements past the last one a plan may write
OLD_BAR = 2e-6      # assert_decode_close's two bars
FLT_MAX = float(np.finfo(np.float32).max)
WIRE_SCALES = [-0.0123, 0.0, -0.0, 1e-42, FLT_MAX, math.inf, math.nan]
SEEDS = [0, 65535, 321, 7, 40000]
_FILL = None


def _fill_word():
    global _FILL
    if _FILL is None:
        _FILL = int(torch.full((1,), float("nan"), dtype=torch.float32).view(torch.int32)[0])
    return _FILL


def _span(plan):
    """Elements of an output arena that covers every slice's padded length."""
    return max([o + sum(d) for o, d in zip(plan.elem_offsets, plan.dims)] + [plan.arena_numel]) + PAD


def _decode(plan, planes, seeds, scales, base=None):
    y = torch.full((_span(plan),), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
    plan.decode(planes, seeds, scales, y, ws, base=base)
    torch.cuda.synchronize()
    return y


def _assert_words(plan, y, want, valid, what, nan=None):
    """y (float32, _span(plan)) against want (int32 words) where valid, against
    the NaN fill elsewhere; where `nan` is set a NaN of any payload is wanted."""
    got = y.view(torch.int32)
    n = want.numel()
    ok = torch.where(valid, got[:n] == want, got[:n] == _fill_word())
    if nan is not None:
        ok = torch.where(nan, torch.isnan(y[:n]), ok)
    tail_ok = bool((got[n:] == _fill_word()).all())
    if bool(ok.all()) and tail_ok:
        return
    bad = torch.nonzero(~ok).reshape(-1)
    offs = np.asarray(plan.elem_offsets)
    head = []
    for i in bad[:16].tolist():
        t = int(np.searchsorted(offs, i, side="right")) - 1
        e = i - int(offs[t])
        head.append((t, e, float(y[i]), float(want[i:i + 1].view(torch.float32)[0]) if bool(valid[i]) else "fill",
                     e >> 15, e & 63))
    raise AssertionError(f"{what}: {bad.numel()} of {n} words differ (written past the arena: {not tail_ok}); "
                         f"(tensor, index, got, want, tile, lane): {head}")


def _base(numel, seed=22):
    return torch.empty(numel, device=DEV).normal_(0, 1.0, generator=torch.Generator(device=DEV).manual_seed(seed))


def _nan_mask(plan, specs, n):
    if not any(math.isnan(r[2]) for _, runs in specs for r in runs):
        return None
    m = torch.zeros(n, dtype=torch.bool, device=DEV)
    for t, (_, runs) in enumerate(specs):
        Ps, Ls = O.slice_plan(plan.numels[t])
        src = plan.elem_offsets[t]
        for ln, r in zip(Ls, runs):
            if math.isnan(r[2]):
                m[src:src + ln] = True
            src += ln
    return m


def _run(plan, specs, bits, what, add=True, planes_view=None):
    """Build the Walsh batch `specs` for `plan`, decode it (and decode it onto
    a base when add) and hold every word.  planes_view(planes) -> the tensor
    to hand to the decoder (part 5).  -> (y, want, valid)."""
    planes, scales, seeds, want, valid = W.build_batch(plan, specs, bits, DEV)
    nan = _nan_mask(plan, specs, want.numel())
    if planes_view is not None:
        planes = planes_view(planes)
    y = _decode(plan, planes, seeds, scales)
    _assert_words(plan, y, want, valid, what, nan)
    if add:
        base = _base(y.numel())
        y2 = _decode(plan, planes, seeds, scales, base=base)
        want2 = (base[:want.numel()] + want.view(torch.float32)).view(torch.int32)
        _assert_words(plan, y2, want2, valid, what + " (decode_add)", nan)
        del base, y2, want2
    return y, want, valid


def _ks(bits):
    nv = 1 << bits
    return [0, nv // 2 - 1, nv // 2, nv - 1]


def _ids(v):
    return "_".join(map(str, v)) if isinstance(v, list) else f"b{v}"


def _names(plan):
    return [l["name"] for l in plan.launches(False)]


# --------------------------------------------------------- 1. Walsh planes ---
SMALL = [[8], [64], [1024], [2048], [1 << 15]]


def _small_specs(bits, ks):
    """(numels, specs): a tensor for every class of SMALL x k x j_set(p), each
    with its own seed (0 and 65535 among them), scales of both signs."""
    numels, specs = [], []
    for (P,) in SMALL:
        for k in ks:
            for j in W.j_set(P.bit_length() - 1):
                t = len(specs)
                seed = (0, 65535)[t] if t < 2 else (t * 7919 + 13) % 65536
                specs.append((seed, [(k, j, (0.0123 if t % 3 else -1.75) * (1 + t % 5))]))
                numels.append(P)
    return numels, specs


@pytest.mark.parametrize("bits", range(1, 9))
def test_walsh_small_classes(bits):
    """One plan per width holds a tensor for every k of the lower half of the
    table (the mirror is the other bin of the run) x j_set(p) at [8], [64],
    [1024], [2048] and [1 << 15]: the small-set launch, one decode call.  A
    second plan adds a [1 << 16] and a [1 << 18] tensor (two column heights:
    the small-set launch fused into the k_col_multi launch) and a third runs one launch per size class (k_dec_tiny,
    k_dec_small<11>, k_dec_small<15>), both over the outermost and the
    innermost k."""
    from openfl_amd.codec import EdenPlan
    numels, specs = _small_specs(bits, range(1 << (bits - 1)))
    plan = EdenPlan(numels, bits)
    assert plan.dims == [[n] for n in numels]
    assert any(n.endswith("k_dec_sset") for n in _names(plan)), _names(plan)
    _run(plan, specs, bits, f"small classes b={bits}")
    del plan
    numels, specs = _small_specs(bits, sorted({0, (1 << (bits - 1)) - 1}))
    big = [(321, [((1 << bits) - 1, 0x5A5A, 0.5)]), (7, [(0, 0x2F0F1, -0.25)])]  # two column heights: k_col_multi
    plan = EdenPlan(numels + [1 << 16, 1 << 18], bits)
    assert any(n.endswith("k_dec_colm_set") for n in _names(plan)), _names(plan)
    _run(plan, specs + big, bits, f"small classes fused b={bits}")
    plan = EdenPlan(numels, bits, sset=0)
    assert {"ofl::k_dec_tiny", "ofl::k_dec_small<11>", "ofl::k_dec_small<15>"} <= set(_names(plan)), _names(plan)
    _run(plan, specs, bits, f"small classes, a launch per class b={bits}")


LARGE = [[1 << 16], [1 << 18], [1 << 21, 8], [1 << 20, 1 << 17], [1 << 23], [1 << 25], [1 << 26]]


def _large_specs(dims, bits, i):
    """Combination i of 5 for one tensor: the slices get different k, j and scale."""
    # above 2^24 the sign words (hashed on one host thread) are shared: seeds 0 and 1
    seed = (i & 1) if max(dims) > 1 << 24 else SEEDS[i % 5]
    runs = []
    for q, P in enumerate(dims):
        p = P.bit_length() - 1
        js = [P - 1, (1 << 14) % P, (1 << 15) % P, 1 << (p - 1), int(np.random.default_rng([77, p, bits]).integers(P))]
        runs.append((_ks(bits)[(i + q) % 4], js[(i + 2 * q + (bits == 3)) % 5],
                     (0.0123, -0.37, 2.5)[(i + q) % 3] * (1 + q)))
    return seed, runs


@pytest.mark.parametrize("bits", [8, 3], ids=_ids)
@pytest.mark.parametrize("dims", LARGE, ids=_ids)
def test_walsh_large_classes(dims, bits):
    """Default plans: one column level ([1 << 16], [1 << 18]), odd plane rows
    ([1 << 21, 8]), two slices ([1 << 20, 1 << 17]), two column levels
    ([1 << 23]), the interleaved layout ([1 << 25]) and the five-pass split
    ([1 << 26]).  Four combinations, each decoded plainly and with base=
    (eight decodes): combination i gives slice q the k number (i + q) % 4 of
    {0, 2^(b-1) - 1, 2^(b-1), 2^b - 1} and the j number (i + 2 q + bit) % 5
    of {P - 1, 2^14, 2^15, 2^(p-1), one random}, bit = 0 at 8 bits and 1 at
    3: a single-slice class sees every k and, over its two widths, every j;
    the other 16 of the 4 x 5 pairs of k and j are not run."""
    from openfl_amd.codec import EdenPlan
    plan = EdenPlan([sum(dims)], bits)
    assert plan.dims == [dims]
    if dims == [1 << 26]:
        assert any(l["expl"] for l in plan.launches(False))
    for i in range(4):
        _run(plan, [_large_specs(dims, bits, i)], bits, f"{dims} b={bits} combination {i}")
    torch.cuda.empty_cache()


@pytest.mark.parametrize("bits", range(1, 9))
def test_walsh_persistent_rows(bits):
    """k_dec_rowA and k_dec_rowC (row2 = 0, pair = 0), one 2^18 slice, every
    width, every k of _ks."""
    from openfl_amd.codec import EdenPlan
    dims = [1 << 18]
    plan = EdenPlan(dims, bits, wave_mib=4096, streams=1, row2=0, pair=0)
    rows = {l["name"].split("<")[0] for l in plan.launches(False) if "_row" in l["name"]}
    assert rows == {"ofl::k_dec_rowA", "ofl::k_dec_rowC"}, rows
    P = dims[0]
    js = [P - 1, 1 << 14, 1 << 15, 1 << 17, 0x2F0F1]
    for i, k in enumerate(sorted(set(_ks(bits)))):
        _run(plan, [(SEEDS[i], [(k, js[(i + bits) % 5], (0.0123, -0.37)[i & 1])])], bits,
             f"persistent rows b={bits} k={k}")


# ------------------------------------------------- 2. ragged and batches ---
@pytest.mark.parametrize("bits", [8, 3], ids=_ids)
@pytest.mark.parametrize("n", [120_003, (1 << 23) + 70_001])
def test_walsh_ragged(n, bits):
    """120 003 of 2^17 and [2^23, 2^17] with 70 001 valid in the last slice
    (its fourth row tile has no valid output); both lengths end inside a
    float4.  The written prefix is exact, and the padding of the slice (the
    arena is allocated to the padded length and beyond) keeps its NaN fill."""
    from openfl_amd.codec import EdenPlan
    dims, lens = O.slice_plan(n)
    assert lens[-1] % 4 and lens[-1] < dims[-1]
    if n > 1 << 23:
        assert lens[-1] <= 3 << 15 < dims[-1]
    plan = EdenPlan([n], bits)
    assert plan.dims == [dims]
    for i in range(3):
        seed, runs = _large_specs(dims, bits, i)
        y, want, valid = _run(plan, [(SEEDS[i], runs)], bits, f"ragged n={n} b={bits} combination {i}")
        assert int(valid.sum()) == n and y.numel() >= sum(dims) + PAD


@pytest.mark.parametrize("wave_mib", [None, 0.5])
def test_walsh_batch(wave_mib):
    """Five Walsh tensors of different classes in one plan, with the default
    waves and with 0.5 MiB waves."""
    from openfl_amd.codec import EdenPlan
    bits = 8
    all_dims = [[1 << 16], [2048], [1 << 18], [1 << 20, 1 << 17], [64]]
    plan = EdenPlan([sum(d) for d in all_dims], bits, wave_mib=wave_mib)
    assert plan.dims == all_dims and (plan.n_waves > 1 if wave_mib else plan.n_waves == 1)
    specs = []
    for t, dims in enumerate(all_dims):
        _, runs = _large_specs(dims, bits, t)
        specs.append((SEEDS[t], runs))
    _run(plan, specs, bits, f"batch wave_mib={wave_mib}")


# ------------------------------------------------------ 3. foreign planes ---
FOREIGN = [[2048], [1 << 16], [1 << 21, 8], [1 << 23], [1 << 26]]
FOREIGN_SEED = 321


def _foreign_bins(kind, dims, bits, g):
    Ptot, nv = sum(dims), 1 << bits
    if kind == "uniform":
        return torch.randint(0, nv, (Ptot,), dtype=torch.int32, device=DEV, generator=g)
    if kind == "sea":
        bins = torch.randint(nv // 2 - 1, nv // 2 + 1, (Ptot,), dtype=torch.int32, device=DEV, generator=g)
        at = torch.randperm(min(Ptot, 1 << 20), device=DEV, generator=g)[:64] * (Ptot // min(Ptot, 1 << 20))
        bins[at] = torch.randint(0, 2, (64,), dtype=torch.int32, device=DEV, generator=g) * (nv - 1)
        return bins
    assert kind == "gauss"
    Bt = torch.from_numpy(O.tables(bits)[1]).to(DEV)
    z = torch.empty(Ptot, dtype=torch.float32, device=DEV).normal_(generator=g)
    return torch.bucketize(z, Bt, out_int32=True)


def _decode64(bins, dims, bits, scales, seed):
    """The fp64 decode on the device: eden_exact.unrotate of C[bins], times the scale."""
    C = torch.from_numpy(O.tables(bits)[0].astype(np.float64)).to(DEV)
    out, off = [], 0
    for P, sc in zip(dims, scales):
        out.append(X.unrotate(C[bins[off:off + P].long()], seed).mul_(float(np.float32(sc))))
        off += P
    return torch.cat(out) if len(out) > 1 else out[0]


def _errors(y, ref):
    e = y.double() - ref
    rel = float(torch.linalg.vector_norm(e) / torch.linalg.vector_norm(ref))
    mx = float(e.abs().max() / ref.abs().max())
    return rel, mx


def _foreign(kind, dims, bits):
    """-> (bins, planes, scales (list), the fp64 decode, the oracle's (rel, max) against it)."""
    g = torch.Generator(device=DEV).manual_seed(1000 * bits + len(kind) + sum(dims) % 997)
    bins = _foreign_bins(kind, dims, bits, g)
    planes = X.expected_planes(bins, dims, bits)
    scales = [0.01 * 3.7 ** q for q in range(len(dims))]
    ref = _decode64(bins, dims, bits, scales, FOREIGN_SEED)
    yo = O.decompress(planes.cpu().numpy(), sum(dims), scales, dims, FOREIGN_SEED, bits)
    return bins, planes, scales, ref, _errors(torch.from_numpy(yo).to(DEV), ref)


def _gpu_decode_planes(plan, planes, scales):
    sd = torch.tensor([FOREIGN_SEED], dtype=torch.int32, device=DEV)
    sc = torch.tensor(scales, dtype=torch.float32, device=DEV)
    return _decode(plan, planes, sd, sc)


@pytest.mark.parametrize("bits", [8, 3], ids=_ids)
@pytest.mark.parametrize("dims", FOREIGN, ids=_ids)
@pytest.mark.parametrize("kind", ["uniform", "sea"])
def test_foreign_planes_vs_fp64(kind, dims, bits):
    """Planes no encoder writes (every bin, both extremes, in every lane; or
    64 extreme bins in a sea of the two central ones) against the fp64
    decode, within 4 x the C oracle's own error on the same planes."""
    from openfl_amd.codec import EdenPlan
    n = sum(dims)
    _, planes, scales, ref, (orel, omx) = _foreign(kind, dims, bits)
    plan = EdenPlan([n], bits)
    assert plan.dims == [dims]
    y = _gpu_decode_planes(plan, planes, scales)
    assert bool(torch.isnan(y[n:]).all())
    rel, mx = _errors(y[:n], ref)
    print(f"[foreign {kind} {dims} b={bits}] rel L2 {rel:.2e} (oracle {orel:.2e})  "
          f"max {mx:.2e} (oracle {omx:.2e})", flush=True)
    assert rel <= 4 * orel and mx <= 4 * omx, (rel, orel, mx, omx)
    del y, ref, planes
    torch.cuda.empty_cache()


@pytest.mark.parametrize("bits", [8, 3], ids=_ids)
@pytest.mark.parametrize("dims", FOREIGN, ids=_ids)
@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_constant_planes_exact(byte, dims, bits):
    """Every plane byte 0x00 (bin 0 everywhere) or 0xFF (bin 2^b - 1): Walsh
    planes with j = 0, so every word is known."""
    from openfl_amd.codec import EdenPlan
    plan = EdenPlan([sum(dims)], bits)
    k = 0 if byte == 0 else (1 << bits) - 1
    spec = (FOREIGN_SEED, [(k, 0, 0.01 * 3.7 ** q) for q in range(len(dims))])
    seen = []

    def check(planes):
        seen.append(bool((planes == byte).all()))
        return planes
    _run(plan, [spec], bits, f"planes of 0x{byte:02X} {dims} b={bits}", planes_view=check)
    assert seen == [True]
    torch.cuda.empty_cache()


def test_one_moved_bin_at_2_26():
    """Why this file exists.  Gaussian bins at [1 << 26], 8 bits; one element
    (in the middle of a row tile, at a central bin, where the centroids lie
    closest: 0.01689 apart) moved to the neighbouring bin.  Against the fp64
    decode of the unmoved planes the decoder's output of the moved planes
      * is refused by the bar of test_foreign_planes_vs_fp64 (4 x the oracle's
        own error) by a factor above 2, in relative L2 and in max error;
      * is off by what the dilution predicts, delta / (sqrt(P) rms C[bins]) =
        2.06e-6 in relative L2 (asserted within 5 %), and by as much in max
        error over max |ref| (the fault arrives as +-delta / sqrt(P) at every
        output, and max |ref| is about 5.5 rms as well): 2.07e-6 and 2.08e-6
        measured.
    The suite's 2e-6 bars (assert_decode_close) therefore do NOT pass this
    fault at 2^26: they sit 4 % below it (asserted: both figures exceed
    OLD_BAR), and the fault falls under them from 2^27 on (the same
    prediction, asserted: 1.46e-6 at 2^27, 7.3e-7 at 2^29).  Those bars see a
    wrong centroid in slices up to 2^26 only, and by 4 % there; the new bar
    has a factor 2.2 in hand at 2^26 and sees it up to 2^28."""
    from openfl_amd.codec import EdenPlan
    dims, bits = [1 << 26], 8
    bins, planes, scales, ref, (orel, omx) = _foreign("gauss", dims, bits)
    plan = EdenPlan(dims, bits)
    y = _gpu_decode_planes(plan, planes, scales)
    rel0, mx0 = _errors(y[:dims[0]], ref)
    assert rel0 <= 4 * orel and mx0 <= 4 * omx, (rel0, orel, mx0, omx)
    at = (1234 << 15) + 16_411
    cand = torch.nonzero(bins[at:at + 4096] == 127).reshape(-1)
    e = at + int(cand[0])
    bins[e] = 128
    del planes, y
    moved = X.expected_planes(bins, dims, bits)
    y = _gpu_decode_planes(plan, moved, scales)
    rel, mx = _errors(y[:dims[0]], ref)
    print(f"[one moved bin 2^26] unmoved rel L2 {rel0:.2e} max {mx0:.2e}; moved rel L2 {rel:.2e} max {mx:.2e}; "
          f"oracle {orel:.2e} / {omx:.2e}", flush=True)
    assert rel > 2 * 4 * orel and mx > 2 * 4 * omx, (rel, orel, mx, omx)
    C = O.tables(bits)[0].astype(np.float64)
    rms = math.sqrt(float(torch.from_numpy(C).to(DEV)[bins.long()].square().mean()))
    predicted = (C[128] - C[127]) / (math.sqrt(dims[0]) * rms)
    assert abs(rel / predicted - 1) <= 0.05, (rel, predicted)
    assert rel > OLD_BAR and mx > OLD_BAR, (rel, mx)
    assert predicted / math.sqrt(2) < OLD_BAR  # the same fault in a 2^27 slice
    del y, ref, moved, bins
    torch.cuda.empty_cache()


# ------------------------------------------------- 4. scales from the wire ---
@pytest.mark.parametrize("scale", WIRE_SCALES, ids=lambda s: repr(s))
@pytest.mark.parametrize("dims", [[64], [2048], [1 << 16], [1 << 23]], ids=_ids)
def test_wire_scales(dims, scale):
    """A scale k_finalize would not write, on the tiny, small, one-level and
    two-level kernels, 8 and 3 bits, with and without base=."""
    from openfl_amd.codec import EdenPlan
    P = dims[0]
    for bits, k, j in ((8, 255, P - 1), (8, 131, (1 << 14) % P + 5), (3, 3, P // 2)):
        plan = EdenPlan(dims, bits)
        _run(plan, [(SEEDS[bits % 5], [(k, j, scale)])], bits, f"scale {scale!r} {dims} b={bits}")


# ----------------------------------------------- 5. planes pointer alignment ---
ALIGN_CASES = {
    "one_level": dict(numels=[1 << 16]),
    "persistent_rows": dict(numels=[1 << 18], wave_mib=4096, streams=1, row2=0, pair=0),
    "odd_rows": dict(numels=[(1 << 21) + 8]),
    "two_levels": dict(numels=[1 << 23]),
    "small_set": dict(numels=[8, 64, 1024, 2048, 1 << 15, 8, 2048]),
}


def _offset_view(nbytes, off):
    """-> (buffer of 0xA5, its view of nbytes that starts `off` bytes in)."""
    buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + nbytes]
    assert view.data_ptr() % 8 == off % 8 and view.is_contiguous()
    return buf, view


@pytest.mark.parametrize("off", [1, 3, 4, 7])
@pytest.mark.parametrize("case", list(ALIGN_CASES), ids=str)
def test_planes_pointer_alignment(case, off):
    """ofl_eden_decode_add and ofl_eden_encode with a planes pointer `off`
    bytes into its allocation (a uint8_t* of any alignment is valid: include/
    ofl_codec.h): the decode equals the aligned one and the Walsh
    expectation; the encode writes the aligned call's bytes and scales and
    leaves the 0xA5 before and after its range alone; so does
    ofl_eden_encode_wavg against its own aligned call."""
    from openfl_amd import _lib
    from openfl_amd.codec import EdenPlan
    kw = dict(ALIGN_CASES[case])
    numels = kw.pop("numels")
    bits = 8 if case != "small_set" else 5
    plan = EdenPlan(numels, bits, **kw)
    if case == "persistent_rows":
        rows = {l["name"].split("<")[0] for l in plan.launches(False) if "_row" in l["name"]}
        assert rows == {"ofl::k_dec_rowA", "ofl::k_dec_rowC"}, rows
    specs = [(SEEDS[t % 5], _large_specs(d, bits, t + off)[1]) for t, d in enumerate(plan.dims)]
    y0, want, valid = _run(plan, specs, bits, f"{case}, aligned", add=False)

    def shifted(planes):
        buf, view = _offset_view(planes.numel(), off)
        view.copy_(planes)
        return view
    y1, _, _ = _run(plan, specs, bits, f"{case}, planes + {off}", planes_view=shifted)
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))
    # encode: Gaussian input into an aligned buffer and into the offset view
    x = _base(plan.arena_numel, seed=5).mul_(0.01)
    seeds = torch.tensor([s for s, _ in specs], dtype=torch.int32, device=DEV)
    ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
    out = []
    for o in (0, off):
        buf, view = _offset_view(plan.planes_bytes, o)
        s = torch.full((plan.n_slices,), float("nan"), dtype=torch.float32, device=DEV)
        plan.encode(x, seeds, view, s, ws)
        torch.cuda.synchronize()
        assert bool((buf[:o] == 0xA5).all()) and bool((buf[o + plan.planes_bytes:] == 0xA5).all()), (case, o)
        out.append((view, s))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert bool(torch.isfinite(out[0][1]).all())
    # ofl_eden_encode_wavg, aligned and into the offset view: two collaborators
    # that both hold x, weights 0.5 / 0.5, no base, the delta arena = x
    xs = [x, x.clone()]
    ptrs = torch.tensor([t.data_ptr() for t in xs], dtype=torch.int64, device=DEV)
    w = torch.tensor([0.5, 0.5], dtype=torch.float64, device=DEV)
    wout = []
    for o in (0, off):
        buf, view = _offset_view(plan.planes_bytes, o)
        s = torch.full((plan.n_slices,), float("nan"), dtype=torch.float32, device=DEV)
        _lib.check(_lib.lib().ofl_eden_encode_wavg(plan.handle, ptrs.data_ptr(), w.data_ptr(), 2,
                                                   ctypes.c_double(1.0), None, x.data_ptr(), seeds.data_ptr(),
                                                   view.data_ptr(), s.data_ptr(), ws.data_ptr(), ws.numel(), None))
        torch.cuda.synchronize()
        assert bool((buf[:o] == 0xA5).all()) and bool((buf[o + plan.planes_bytes:] == 0xA5).all()), (case, o)
        wout.append((view, s))
    assert torch.equal(wout[0][0], wout[1][0]) and torch.equal(wout[0][1], wout[1][1])
    assert bool(torch.isfinite(wout[0][1]).all())
    for po, pb in zip(plan.planes_offsets, plan.planes_nbytes):
        assert bool((out[0][0][po:po + pb] != 0xA5).any())
