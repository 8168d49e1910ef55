"""GPU parity: the HIP codec (libofl_codec.so) against the reference's golden
outputs and the CPU oracle, called through the C ABI.

Tolerances (written here, checked per test):
  * decode of identical bytes+metadata: relative L2 <= 2e-6 and
    max |err| <= 2e-6 * max|y| (fp32; our normalisation uses exact powers of
    two where the reference divides by float32(sqrt(P)) twice);
  * encode: bins agree on >= 99.9 % of elements (survey bar: 99.8 %), every
    mismatch is a neighbouring bin (|dbin| = 1) -- the FWHT is summed in a
    different order than torch's, so a value sitting on a boundary can round
    to either side; slicing, dims, metadata and plane layout exact;
  * per-slice scales: relative error <= 1e-3 (survey bar), observed ~1e-6.
"""
import threading

import numpy as np
import pytest
import torch

from oracle import eden as O
from tests import golden_io

pytestmark = pytest.mark.gpu

ARR, IDX = golden_io.eden()
CASES = IDX["eden_cases"]
DEV = "cuda:0"
BIN_AGREE = 0.999


def _codec(bits):
    from openfl_amd.codec import EdenCodec
    return EdenCodec(bits, DEV)


def gpu_encode(x, seed, bits):
    c = _codec(bits)
    n = x.size
    plan = c.plan([n])
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV) if n else torch.empty(1, device=DEV)
    sd = torch.tensor([seed], dtype=torch.int32, device=DEV)
    planes, scales = c.encode_arena(plan, xd, sd)
    torch.cuda.synchronize()
    return planes[:plan.planes_bytes].cpu().numpy(), scales[:plan.n_slices].cpu().numpy(), plan.dims[0]


def gpu_decode(planes, total, scales, dims, seed, bits):
    c = _codec(bits)
    plan = c.plan([total], dims=[dims])
    y = c.decode_arena(plan, torch.from_numpy(np.ascontiguousarray(planes)).to(DEV),
                       torch.tensor(np.asarray(scales, np.float32)).to(DEV),
                       torch.tensor([seed], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    return y[:total].cpu().numpy()


def assert_bins_close(planes_a, planes_b, P, bits, agree=BIN_AGREE):
    a, b = O.bins_of(planes_a, P, bits), O.bins_of(planes_b, P, bits)
    assert np.mean(a == b) >= agree, np.mean(a != b)
    assert np.max(np.abs(a - b)) <= 1


def assert_decode_close(y, ref):
    ref = ref.astype(np.float64)
    y = y.astype(np.float64)
    scale = max(np.max(np.abs(ref)), 1e-30)
    assert np.max(np.abs(y - ref)) <= 2e-6 * scale
    if np.linalg.norm(ref) > 0:
        assert np.linalg.norm(y - ref) <= 2e-6 * np.linalg.norm(ref)


def _finite_scales_close(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)
    assert np.all(got[~fin] == ref[~fin])
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-3, atol=0)


# ---------------------------------------------------------------- goldens ---
@pytest.mark.parametrize("case", [c for c in CASES if "planes_key" in c], ids=lambda c: c["tag"])
def test_encode_matches_reference(case):
    x = ARR[case["x_key"]]
    planes, scales, dims = gpu_encode(x, case["seed"], case["bits"])
    assert dims == case["dims"]
    assert planes.size == case["planes_len"]
    assert_bins_close(planes, ARR[case["planes_key"]], sum(dims), case["bits"])
    _finite_scales_close(scales, case["scales"])


@pytest.mark.parametrize("case", [c for c in CASES if "planes_key" in c], ids=lambda c: c["tag"])
def test_decode_matches_reference(case):
    y = gpu_decode(ARR[case["planes_key"]], case["total_dim"], case["scales"], case["dims"],
                   case["seed"], case["bits"])
    if "y_key" in case:
        ref = ARR[case["y_key"]]
        if not np.all(np.isfinite(ref)):
            assert np.array_equal(np.isfinite(y), np.isfinite(ref))
            return
        assert_decode_close(y, ref)
    else:
        s = case["ysample_stride"]
        ys = ARR[case["ysample_key"]]
        assert_decode_close(y[::s][:ys.size], ys)


# --------------------------------------------------- oracle, every kernel class ---
# sizes hitting: tiny (P <= 2^10), small register kernels 2^11..2^14, the
# large path with one column level (p = 15..22 -> M = 2..9) and two levels
# (p = 23..25), multi-slice tensors and ragged tails.
# 120_003 / (1 << 23) + 70_001: a large slice whose valid length ends inside a
# float4 (row-pass tail patch) and, for the latter, a row tile with no valid
# input at all; (1 << 21) + 7: plane rows not 8-byte aligned (byte-wise path).
SIZES = [3, 64, 300, 1000, 2048, 3000, 4096, 8192, 12000, 16384, 16385, 1 << 15, 50_000, 1 << 17,
         120_003, 300_000, 1 << 19, 1 << 20, (1 << 21) + 7, 1 << 22, 1 << 23, (1 << 23) + 70_001,
         (1 << 24) + 12345, 1 << 25]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bits", [8, 3])
def test_encode_decode_vs_oracle(n, bits):
    _check_encode_decode_vs_oracle(n, bits)


# The other bit widths on the large path (the goldens cover 1..8 bits only up
# to 65 537 elements: one tile pair, aligned plane rows): a ragged 2^17 slice,
# plane rows that are not 8-byte aligned (dims [2^21, 8]) and two column
# levels.  Same bars.
@pytest.mark.parametrize("n", [120_003, (1 << 21) + 7, 1 << 23])
@pytest.mark.parametrize("bits", [1, 2, 4, 5, 6, 7])
def test_encode_decode_vs_oracle_bit_widths(n, bits):
    _check_encode_decode_vs_oracle(n, bits)


def _check_encode_decode_vs_oracle(n, bits):
    x = np.random.default_rng(n + bits).standard_normal(n).astype(np.float32) * np.float32(0.01)
    seed = (n * 7 + bits) % 65536
    planes, scales, dims = gpu_encode(x, seed, bits)
    oplanes, oscales, odims, _ = O.compress(x, seed, bits)
    assert dims == odims
    assert_bins_close(planes, oplanes, sum(dims), bits)
    _finite_scales_close(scales, oscales)
    # cross-decode: our decoder on the oracle's (= reference) bytes
    y = gpu_decode(oplanes, n, oscales, odims, seed, bits)
    assert_decode_close(y, O.decompress(oplanes, n, oscales, odims, seed, bits))


@pytest.mark.parametrize("tag", ["zeros", "const", "withinf", "huge", "tiny", "spike"])
def test_edge_cases(tag):
    for bits in (2, 8):
        case = next(c for c in CASES if c["tag"] == f"b{bits}_edge_{tag}")
        x = ARR[case["x_key"]]
        planes, scales, dims = gpu_encode(x, case["seed"], bits)
        ref_planes = ARR[case["planes_key"]]
        ref_scales = np.asarray(case["scales"])
        if tag in ("zeros", "withinf", "tiny"):  # reference zero fallback (:517-525)
            assert np.all(planes == 0) and np.all(scales == 0)
            assert np.array_equal(planes, ref_planes)
        elif tag == "huge":  # norm overflows to inf in fp32 -> all bins at the centre, scale -inf
            assert np.array_equal(planes, ref_planes)
            assert np.array_equal(scales, ref_scales.astype(np.float32))
        else:
            assert_bins_close(planes, ref_planes, sum(dims), bits)
            _finite_scales_close(scales, case["scales"])


def _bins_mismatch_chunked(pa, pb, P, bits, chunk=1 << 24):
    """(mismatching elements, max |dbin|) of two to_bits plane sets, in
    chunks (a 2^29-element unpack would need tens of GiB at once)."""
    L = P // 8
    pa = np.frombuffer(bytes(pa) if not isinstance(pa, np.ndarray) else pa, np.uint8).reshape(bits, L)
    pb = np.frombuffer(bytes(pb) if not isinstance(pb, np.ndarray) else pb, np.uint8).reshape(bits, L)
    bad, worst = 0, 0
    w = (1 << np.arange(bits, dtype=np.int32))[:, None]
    for j0 in range(0, L, chunk // 8):
        j1 = min(L, j0 + chunk // 8)
        if np.array_equal(pa[:, j0:j1], pb[:, j0:j1]):
            continue
        ba = (np.unpackbits(pa[:, j0:j1], axis=1, bitorder="little").astype(np.int32) * w).sum(0)
        bb = (np.unpackbits(pb[:, j0:j1], axis=1, bitorder="little").astype(np.int32) * w).sum(0)
        d = np.abs(ba - bb)
        bad += int(np.count_nonzero(d))
        worst = max(worst, int(d.max()))
    return bad, worst


def _decode_err_chunked(y, ref, chunk=1 << 24):
    """(relative L2, max |err| / max |ref|) in float64, chunked."""
    se = sr = 0.0
    me = mr = 0.0
    for i in range(0, ref.size, chunk):
        r = ref[i:i + chunk].astype(np.float64)
        e = y[i:i + chunk].astype(np.float64) - r
        se += float(np.dot(e, e))
        sr += float(np.dot(r, r))
        me = max(me, float(np.max(np.abs(e))))
        mr = max(mr, float(np.max(np.abs(r))))
    return np.sqrt(se / sr), me / max(mr, 1e-30)


# The five-pass large-slice FWHT (2^26 <= P <= 2^29: two column levels, the
# middle one carrying D2) against the oracle (eden_pipeline.py:451-473 hadamard,
# :403-449 rand_diag, :661-690 to_bits): one 2^26 slice, a 2^27 slice with a
# ragged tail (valid length ends inside a float4), and the Llama-3-8B
# embed_tokens / lm_head tensor 128256 x 4096 (one 2^29 slice).  Same bars as
# above; the encode is run twice over differently pre-filled plane buffers,
# so every plane byte is shown to be written.
@pytest.mark.timeout(900)
@pytest.mark.parametrize("n", [1 << 26, (1 << 27) - 99_997, 128256 * 4096])
def test_five_pass_slices_vs_oracle(n):
    from openfl_amd.codec import EdenPlan
    bits, seed = 8, (n * 13 + 5) % 65536
    x = np.random.default_rng(n % 1000).standard_normal(n).astype(np.float32) * np.float32(0.01)
    c = _codec(bits)
    plan = c.plan([n])
    P = sum(plan.dims[0])
    assert plan.dims[0] == O.slice_plan(n)[0] and max(plan.dims[0]) >= 1 << 26
    xd = torch.from_numpy(x).to(DEV)
    sd = torch.tensor([seed], dtype=torch.int32, device=DEV)
    outs = []
    for fill in (0x00, 0xFF):
        planes = torch.full((plan.planes_bytes,), fill, dtype=torch.uint8, device=DEV)
        scales = torch.full((plan.n_slices,), float("nan"), dtype=torch.float32, device=DEV)
        ws = c.ws.get(plan.ws_bytes, c.device)
        plan.encode(xd, sd, planes, scales, ws)
        torch.cuda.synchronize()
        outs.append((planes.cpu().numpy(), scales.cpu().numpy()))
        del planes, scales
    del xd
    torch.cuda.empty_cache()
    (gp, gs), (gp2, gs2) = outs
    assert np.array_equal(gp, gp2) and np.array_equal(gs, gs2)  # every byte written
    assert gp.size == bits * P // 8
    print(f"[five-pass n={n}] GPU encodes done; oracle compress on {O.get_threads()} threads", flush=True)
    op, osc, odims, _ = O.compress(x, seed, bits)
    assert odims == plan.dims[0] and op.size == gp.size
    bad, worst = _bins_mismatch_chunked(gp, op, P, bits)
    assert bad <= (1 - BIN_AGREE) * P and worst <= 1, (bad, worst)
    _finite_scales_close(gs, osc)
    del gp2, gs2, outs
    # cross-decode the oracle's (= reference) bytes with the HIP decoder
    print(f"[five-pass n={n}] bins {bad} mismatches; decoding", flush=True)
    y = gpu_decode(op, n, osc, odims, seed, bits)
    yo = O.decompress(op, n, osc, odims, seed, bits)
    rel, mx = _decode_err_chunked(y, yo)
    assert rel <= 2e-6 and mx <= 2e-6, (rel, mx)
    # and the end-to-end quantisation error of the HIP round trip is Eden's
    y2 = gpu_decode(gp, n, gs, plan.dims[0], seed, bits)
    e2e, _ = _decode_err_chunked(y2, x)
    assert 5.5e-3 < e2e < 7.5e-3
    torch.cuda.empty_cache()


def test_large_slice_property_2p29():
    """Llama-3-8B embed/lm_head size (one 2^29 slice, 128256 x 4096 elements):
    too big for the oracle in test time, so check size-independent properties:
    8-bit Eden error ~6.4e-3 relative (Gaussian input), decode deterministic,
    linearity of the scale, every plane byte written.  The encode's ground
    truth at this size is tests/test_gpu_eden_exact.py::
    test_designed_exact_five_pass[29-8]: a designed 2^29 input whose planes
    and scale are known exactly, built and compared on the device."""
    n = 128256 * 4096
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.empty(n, device=DEV).normal_(0, 0.01, generator=g)
    c = _codec(8)
    plan = c.plan([n])
    assert plan.dims == [[1 << 29]]
    sd = torch.tensor([999], dtype=torch.int32, device=DEV)
    planes, scales = c.encode_arena(plan, x, sd)
    y1 = c.decode_arena(plan, planes, scales, sd)
    y2 = c.decode_arena(plan, planes, scales, sd)
    torch.cuda.synchronize()
    rel = float(torch.linalg.vector_norm((y1[:n] - x).double()) / torch.linalg.vector_norm(x.double()))
    assert 5.5e-3 < rel < 7.5e-3
    assert torch.equal(y1[:n], y2[:n])
    # scale linearity: decode with 2*scale gives exactly 2*y
    y3 = c.decode_arena(plan, planes, scales * 2, sd)
    torch.cuda.synchronize()
    assert torch.equal(y3[:n], 2 * y1[:n])
    del x, y1, y2, y3, planes
    torch.cuda.empty_cache()


# ------------------------------------------------------ batching / arenas ---
def test_batch_equals_single():
    _check_batch_equals_single([5, 1000, 4096, 70_000, 1 << 20, 3], 8)


# At 3 bits the second plan puts an odd-length plane run (3 * (2^18 + 1) =
# 786 435 bytes) in front of a large tensor.
@pytest.mark.parametrize("numels", [[5, 1000, 4096, 70_000, 1 << 20, 3], [1000, (1 << 21) + 7, 3000, 1 << 20]],
                         ids=["mixed", "odd_plane_runs"])
@pytest.mark.parametrize("bits", [3, 5])
def test_batch_equals_single_bits(bits, numels):
    if len(numels) == 4 and bits == 3:
        from openfl_amd.codec import EdenPlan
        assert EdenPlan(numels, 3).planes_nbytes[1] == 786_435
    _check_batch_equals_single(numels, bits)


def _check_batch_equals_single(numels, bits):
    from openfl_amd.codec import EdenPlan
    rng = np.random.default_rng(11)
    xs = [rng.standard_normal(n).astype(np.float32) for n in numels]
    seeds = [11, 22, 33, 44, 55, 66][:len(numels)]
    plan = EdenPlan(numels, bits)
    arena = torch.zeros(plan.arena_numel, device=DEV)
    for x, off in zip(xs, plan.elem_offsets):
        arena[off:off + x.size] = torch.from_numpy(x).to(DEV)
    c = _codec(bits)
    sd = torch.tensor(seeds, dtype=torch.int32, device=DEV)
    planes, scales = c.encode_arena(plan, arena, sd)
    y = c.decode_arena(plan, planes, scales, sd)
    torch.cuda.synchronize()
    planes, scales, y = planes.cpu().numpy(), scales.cpu().numpy(), y.cpu().numpy()
    for t, (x, s) in enumerate(zip(xs, seeds)):
        p1, s1, d1 = gpu_encode(x, s, bits)
        po, pb = plan.planes_offsets[t], plan.planes_nbytes[t]
        np.testing.assert_array_equal(planes[po:po + pb], p1)
        fs = plan.first_slice[t]
        np.testing.assert_array_equal(scales[fs:fs + len(d1)], s1)
        y1 = gpu_decode(p1, x.size, s1, d1, s, bits)
        off = plan.elem_offsets[t]
        np.testing.assert_array_equal(y[off:off + x.size], y1)


def test_many_large_slices_one_launch():
    """1100 large slices in one plan: more than the row kernels' LDS tile table
    holds (1024), so the persistent walk takes the global-table path; 880 tiny
    tail slices interleaved make slice ids exceed the large-slice count (the
    per-slice norm table is indexed by slice id).  Every tensor must equal its
    own single-tensor encode/decode."""
    from openfl_amd.codec import EdenPlan
    T = 1100
    numels = [65536 + (t % 5) for t in range(T)]
    plan = EdenPlan(numels, 8)
    assert sum(len(d) for d in plan.dims) >= T
    g = torch.Generator(device=DEV).manual_seed(3)
    arena = torch.empty(plan.arena_numel, device=DEV).normal_(0, 0.01, generator=g)
    seeds = [(7 * t + 1) % 65536 for t in range(T)]
    c = _codec(8)
    sd = torch.tensor(seeds, dtype=torch.int32, device=DEV)
    planes, scales = c.encode_arena(plan, arena, sd)
    y = c.decode_arena(plan, planes, scales, sd)
    torch.cuda.synchronize()
    xa = arena.cpu().numpy()
    planes, scales, y = planes.cpu().numpy(), scales.cpu().numpy(), y.cpu().numpy()
    for t in range(T):
        off, n = plan.elem_offsets[t], numels[t]
        x = xa[off:off + n]
        p1, s1, d1 = gpu_encode(x, seeds[t], 8)
        po, pb = plan.planes_offsets[t], plan.planes_nbytes[t]
        np.testing.assert_array_equal(planes[po:po + pb], p1)
        fs = plan.first_slice[t]
        np.testing.assert_array_equal(scales[fs:fs + len(d1)], s1)
        np.testing.assert_array_equal(y[off:off + n], gpu_decode(p1, n, s1, d1, seeds[t], 8))


def test_schedules_bit_identical():
    """The large-slice schedule (waves, one or two streams) orders the passes
    but never changes a value: planes, scales and decoded output are
    bit-identical across schedules, including a slice bigger than the wave,
    two column levels (2^26) and mixed small/tiny slices."""
    from openfl_amd.codec import EdenPlan
    numels = [(1 << 22) + 5, 1 << 16, 3000, (1 << 26) - 1000, 1 << 20, 77, (1 << 23) + (1 << 17), 1 << 22]
    g = torch.Generator(device=DEV).manual_seed(21)
    seeds = [(97 * t + 5) % 65536 for t in range(len(numels))]
    c = _codec(8)
    sd = torch.tensor(seeds, dtype=torch.int32, device=DEV)
    ref = None
    for wave_mib, streams in ((0, 1), (64, 1), (16, 2), (1, 2), (48, 1)):
        plan = EdenPlan(numels, 8, wave_mib=wave_mib, streams=streams)
        if ref is None:
            arena = torch.empty(plan.arena_numel, device=DEV).normal_(0, 0.01, generator=g)
        planes, scales = c.encode_arena(plan, arena, sd)
        y = c.decode_arena(plan, planes, scales, sd)
        torch.cuda.synchronize()
        # the written ranges only (arena alignment gaps are never written)
        out = (torch.cat([planes[o:o + b] for o, b in zip(plan.planes_offsets, plan.planes_nbytes)]),
               scales[:plan.n_slices].clone(),
               torch.cat([y[o:o + n] for o, n in zip(plan.elem_offsets, numels)]))
        if ref is None:
            ref = out
            xs = torch.cat([arena[o:o + n] for o, n in zip(plan.elem_offsets, numels)])
            rel = float(torch.linalg.vector_norm((out[2] - xs).double()) / torch.linalg.vector_norm(xs.double()))
            assert 5.5e-3 < rel < 7.5e-3
        else:
            assert plan.n_waves > 1
            for a, b in zip(out, ref):
                assert torch.equal(a, b), (wave_mib, streams)
    del arena, planes, y, ref
    torch.cuda.empty_cache()


@pytest.mark.parametrize("streams", [1, 2])
def test_fused_small_set_bit_identical(streams):
    """The small-set groups inside a one-wave plan's k_col_multi launch
    (k_*_colm_set, every launch on the caller's stream) give the same planes,
    scales and decoded values as the small-set launch on its own (ResNet-50's
    slice sizes: tiny, small, heights 1..6)."""
    from openfl_amd.codec import EdenPlan
    from openfl_amd.workloads import WORKLOADS, numel
    numels = [numel(s) for _, s in WORKLOADS["resnet50_fp32"]() if numel(s) > 100]
    g = torch.Generator(device=DEV).manual_seed(5)
    sd = torch.tensor([(31 * t + 7) % 65536 for t in range(len(numels))], dtype=torch.int32, device=DEV)
    c = _codec(8)
    outs = {}
    arena = None
    for fuse in (1, 0):
        plan = EdenPlan(numels, 8, streams=streams, fuse=fuse)
        names = [l["name"] for l in plan.launches(True)]
        assert ("ofl::k_enc_colm_set" in names) == (fuse == 1), names
        if arena is None:
            arena = torch.empty(plan.arena_numel, device=DEV).normal_(0, 0.01, generator=g)
        planes, scales = c.encode_arena(plan, arena, sd)
        y = c.decode_arena(plan, planes, scales, sd)
        torch.cuda.synchronize()
        outs[fuse] = (torch.cat([planes[o:o + b] for o, b in zip(plan.planes_offsets, plan.planes_nbytes)]),
                      scales[:plan.n_slices].clone(),
                      torch.cat([y[o:o + n] for o, n in zip(plan.elem_offsets, numels)]))
    for a, b in zip(outs[1], outs[0]):
        assert torch.equal(a, b)


# --------------------------------------------------------- plugin surface ---
@pytest.mark.parametrize("rec", IDX["forward"], ids=lambda r: r["tag"])
def test_pipeline_forward_backward_vs_reference(rec):
    from openfl_amd.pipelines import EdenPipeline
    pipe = EdenPipeline(n_bits=8, dim_threshold=100, device=DEV)
    assert pipe.is_lossy()
    x = ARR["fwx_" + rec["tag"]]
    ref_bytes = ARR["fwb_" + rec["tag"]].tobytes()
    np.random.seed(rec["np_seed"])
    data, md = pipe.forward(x)
    assert md[0]["int_list"] == rec["int_list"]
    if rec["int_to_float"] is None:                   # small tensor: raw fp32 bytes
        assert "int_to_float" not in md[0] and data == ref_bytes
        out = pipe.backward(data, md)                  # reference crashes at == threshold (:808)
        np.testing.assert_array_equal(out, x.astype(np.float32))
        return
    ref_md = dict(rec["int_to_float"])
    assert set(md[0]["int_to_float"]) == set(ref_md)
    assert md[0]["int_to_float"][0] == ref_md[0] and md[0]["int_to_float"][1] == ref_md[1]
    for k in range(3, max(ref_md) + 1, 2):
        assert md[0]["int_to_float"][k] == ref_md[k]
    dims = [int(ref_md[k]) for k in range(3, max(ref_md) + 1, 2)]
    assert_bins_close(np.frombuffer(data, np.uint8), np.frombuffer(ref_bytes, np.uint8), sum(dims), 8)
    # our backward on the REFERENCE's bytes + metadata (cross-decode)
    out = pipe.backward(ref_bytes, [{"int_list": rec["int_list"], "int_to_float": ref_md}])
    assert out.dtype == np.float32 and list(out.shape) == rec["int_list"]
    assert_decode_close(out.reshape(-1), ARR["fwy_" + rec["tag"]].reshape(-1))


def test_pipeline_batch_equals_per_tensor():
    """forward_batch / backward_batch == per-tensor forward / backward: same
    bytes, metadata, np.random draws and decoded arrays (mixed sizes incl.
    raw small tensors, a tensor at the threshold and float64 input)."""
    from openfl_amd.pipelines import EdenPipeline
    rng = np.random.default_rng(8)
    arrays = [rng.standard_normal((64, 3, 7, 7)).astype(np.float32), rng.standard_normal(100).astype(np.float32),
              rng.standard_normal(5).astype(np.float32), rng.standard_normal((1000, 300)).astype(np.float32),
              rng.standard_normal(70_001), rng.standard_normal((2048, 2048)).astype(np.float32) * 0.01]
    pipe = EdenPipeline(n_bits=8, device=DEV)
    np.random.seed(123)
    ref = [pipe.forward(a) for a in arrays]
    after = np.random.randint(0, 2 ** 31)
    np.random.seed(123)
    got = pipe.forward_batch(arrays)
    assert np.random.randint(0, 2 ** 31) == after
    for (b1, m1), (b2, m2) in zip(ref, got):
        assert b1 == b2 and m1 == m2
    ys_ref = [pipe.backward(b, [dict(m[0])]) for b, m in ref]
    ys = pipe.backward_batch([(b, [dict(m[0])]) for b, m in got])
    for a, b in zip(ys_ref, ys):
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
        np.testing.assert_array_equal(a, b)


def test_pipeline_float32_metadata_roundtrip():
    """Metadata as it arrives off the wire: float32 values (base.proto:22)."""
    from openfl_amd.pipelines import EdenPipeline
    pipe = EdenPipeline(n_bits=4, device=DEV)
    x = np.random.default_rng(2).standard_normal((300, 17)).astype(np.float32)
    data, md = pipe.forward(x)
    md32 = [{"int_list": list(md[0]["int_list"]),
             "int_to_float": {k: float(np.float32(v)) for k, v in md[0]["int_to_float"].items()}}]
    out = pipe.backward(data, md32)
    assert out.shape == x.shape
    rel = np.linalg.norm(out - x) / np.linalg.norm(x)
    assert rel < 0.12  # 4-bit Eden


def test_pipeline_concurrent_threads():
    """forward/backward may run concurrently on one instance (gRPC thread pool)."""
    from openfl_amd.pipelines import EdenPipeline
    pipe = EdenPipeline(n_bits=8, device=DEV)
    rng = np.random.default_rng(9)
    xs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(200, 300_000, 24)]
    np.random.seed(0)
    ref = [pipe.forward(x) for x in xs]
    ref_out = [pipe.backward(d, [dict(m[0])]) for d, m in ref]
    results = [None] * len(xs)

    def work(i):
        d, m = ref[i]
        results[i] = pipe.backward(d, [dict(m[0])])

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(xs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for a, b in zip(results, ref_out):
        np.testing.assert_array_equal(a, b)


def test_step_graph_replay_bit_identical():
    """EdenStepGraph (a captured hipGraph of a plan's encode + decode, the
    side-stream fork/join included) replays the same bytes and values as the
    eager launches, on a mixed set (tiny, small and large slices, two wave
    streams plus the small-slice stream)."""
    from openfl_amd.codec import EdenPlan, EdenStepGraph
    numels = [50_000, 3000, 1 << 20, 700, (1 << 22) + 123, 1 << 15]
    plan = EdenPlan(numels, 8, wave_mib=8, streams=2)
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.empty(plan.arena_numel, device=DEV).normal_(0, 0.01, generator=g)
    seeds = torch.tensor([11, 12, 13, 14, 15, 16], dtype=torch.int32, device=DEV)
    ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
    # zero-filled: the alignment gaps between tensors' plane runs are never written
    p0 = torch.zeros(plan.planes_bytes, dtype=torch.uint8, device=DEV)
    s0 = torch.zeros(plan.n_slices, dtype=torch.float32, device=DEV)
    y0 = torch.zeros_like(x)
    plan.encode(x, seeds, p0, s0, ws)
    plan.decode(p0, seeds, s0, y0, ws)
    p1, s1, y1 = torch.zeros_like(p0), torch.zeros_like(s0), torch.zeros_like(x)
    gr = EdenStepGraph(plan, x, seeds, p1, s1, y1, ws)
    for fill in (p1, s1, y1):
        fill.zero_()
    gr.replay()
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(p0, p1) and torch.equal(s0, s1) and torch.equal(y0, y1)


def test_step_graphs_built_concurrently():
    """Two threads building EdenStepGraphs on one device at once (the graphs
    share the device's capture stream; construction is serialised by its
    lock): both captures succeed and replay the eager bytes."""
    import threading
    from openfl_amd.codec import EdenPlan, EdenStepGraph
    numels = [50_000, 1 << 20, 3000]
    plan = EdenPlan(numels, 8, wave_mib=8, streams=2)
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.empty(plan.arena_numel, device=DEV).normal_(0, 0.01, generator=g)
    seeds = torch.tensor([5, 6, 7], dtype=torch.int32, device=DEV)
    ref = (torch.zeros(plan.planes_bytes, dtype=torch.uint8, device=DEV), torch.zeros_like(x))
    ws0 = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
    s0 = torch.zeros(plan.n_slices, dtype=torch.float32, device=DEV)
    plan.encode(x, seeds, ref[0], s0, ws0)
    plan.decode(ref[0], seeds, s0, ref[1], ws0)
    torch.cuda.synchronize()
    outs, errs = [], []

    def build():
        try:
            torch.cuda.set_device(DEV)
            p = torch.zeros_like(ref[0])
            y = torch.zeros_like(x)
            s = torch.zeros_like(s0)
            ws = torch.empty_like(ws0)
            gr = EdenStepGraph(plan, x, seeds, p, s, y, ws)
            p.zero_()
            y.zero_()
            gr.replay()
            torch.cuda.current_stream().synchronize()
            outs.append((p, y, gr))
        except Exception as e:  # noqa: BLE001 -- reported below
            errs.append(e)
    ts = [threading.Thread(target=build) for _ in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    torch.cuda.synchronize()
    for p, y, _ in outs:
        assert torch.equal(p, ref[0]) and torch.equal(y, ref[1])


@pytest.mark.parametrize("setting", ["cuda:all", "two_slots_one_gpu"])
def test_pipeline_multi_device_threads(setting):
    """device naming several GPUs: each calling thread is bound to one of them
    round-robin (codec.ThreadDevices) -- concurrent forward and backward calls
    from unchanged callers (the gRPC pool, aggregator_server.py:305) give the
    bytes, metadata and values of the single-device path.  "cuda:all" = every
    visible GPU (plain "cuda" is the current device only); on a one-GPU box the same device is also listed twice, so two
    slots (separate codecs, plans, workspaces) share it."""
    from openfl_amd.pipelines import EdenPipeline
    dev = "cuda:all" if setting == "cuda:all" else [DEV, DEV]
    multi = EdenPipeline(n_bits=8, device=dev)
    single = EdenPipeline(n_bits=8, device=DEV)
    eden = multi.transformers[0].eden
    assert len(eden.devices) == (torch.cuda.device_count() if setting == "cuda:all" else 2)
    assert len(EdenPipeline(n_bits=8, device="cuda").transformers[0].eden.devices) == 1
    rng = np.random.default_rng(19)
    xs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(200, 600_000, 16)]
    seeds = rng.integers(1, 2 ** 16, len(xs))
    ref, ref_out = [], []
    for x, s in zip(xs, seeds):
        planes, scales, dims, tot = single.transformers[0].eden.compress(x, int(s))
        ref.append((planes.tobytes(), scales, dims, tot))
    for (b, sc, dims, tot), s in zip(ref, seeds):
        md = {0: float(s), 1: float(tot)}
        for k, (a, d) in enumerate(zip(sc, dims)):
            md[2 + 2 * k], md[3 + 2 * k] = a, float(d)
        ref_out.append(single.transformers[0].eden.decompress(np.frombuffer(b, np.uint8), md))
    enc, dec, slots = [None] * len(xs), [None] * len(xs), [None] * len(xs)

    def work(i):
        planes, scales, dims, tot = eden.compress(xs[i], int(seeds[i]))
        enc[i] = (planes.tobytes(), scales, dims, tot)
        md = {0: float(seeds[i]), 1: float(tot)}
        for k, (a, d) in enumerate(zip(scales, dims)):
            md[2 + 2 * k], md[3 + 2 * k] = a, float(d)
        dec[i] = eden.decompress(np.frombuffer(enc[i][0], np.uint8), md)
        slots[i] = eden._thread_devices.slot()

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(xs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i in range(len(xs)):
        assert enc[i][0] == ref[i][0] and enc[i][1:] == ref[i][1:]
        np.testing.assert_array_equal(dec[i], ref_out[i])
    assert sorted(set(slots)) == list(range(len(eden.devices)))  # every device got threads


def test_row2_variants_bit_identical():
    """The two-blocks-per-CU row kernels (k_enc_rowA2 / k_dec_rowA2 /
    k_dec_rowC2, ofl_eden_plan_set_row2) butterfly the index bits in the same
    order as the persistent ones and load, sum and store the same values: planes,
    scales and decoded values are bit-identical, for 3-pass (incl. the
    interleaved 2^25 layout) and 5-pass slices, ragged tails and decode_add.
    The same with tile pairs (ofl_eden_plan_set_pair: a block hashes the D1
    words of a tile and of the one 2^(p-3) up once), forced on and off, and
    with 2 MiB waves (every 2^18..2^22 slice in its own paired launch); at
    64 MiB waves the 2^26 slice runs split into MALL sub-waves (passes 1-2
    and 4-5 per sub-block, explicit tile lists), paired and unpaired."""
    from openfl_amd.codec import EdenPlan
    numels = [(1 << 26) + 777, 1 << 25, (1 << 22) + 12345, (1 << 16) + 5, 3000, (1 << 18) + 3, (1 << 17) + 1,
              (1 << 19) - 7]
    g = torch.Generator(device=DEV).manual_seed(21)
    outs = []
    for row2, pair, wave in ((0, 0, 4096), (1, 0, 4096), (1, 1, 4096), (1, 1, 2), (-1, -1, 2), (-1, -1, 64),
                             (-1, 0, 64)):
        plan = EdenPlan(numels, 8, wave_mib=wave, streams=1, row2=row2, pair=pair)
        for enc in (True, False):  # the plan runs what its setting says
            rows = [l for l in plan.launches(enc) if "_row" in l["name"]]
            sub = [l for l in rows if l["expl"]]
            signs = [l for l in sub if ("_rowA2" in l["name"] if enc else "_rowC2" in l["name"])]
            if wave == 64:  # the 2^26 slice in sub-waves, paired unless pair = 0
                assert len(sub) == 8 and len(signs) == 4
                assert all(l["paired"] == (pair != 0) for l in signs)
                assert not any(l["paired"] for l in sub if l not in signs)
            else:
                assert not sub
            if pair == 0 or row2 == 0:
                assert not any(l["paired"] for l in rows)
            if row2 == 0:
                assert not any(n in l["name"] for l in rows for n in ("_rowA2", "k_dec_rowC2"))
            if row2 == 1:
                assert not any(l["name"].endswith(("_rowA", "_rowC")) for l in rows)
            if (row2, pair) == (1, 1):
                assert any(l["paired"] for l in rows)
        x = torch.empty(plan.arena_numel, device=DEV).normal_(0, 0.01, generator=g.manual_seed(21))
        base = torch.empty(plan.arena_numel, device=DEV).normal_(0, 1.0, generator=g.manual_seed(22))
        seeds = torch.tensor([5, 6, 7, 8, 9, 10, 11, 12], dtype=torch.int32, device=DEV)
        ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
        p = torch.full((plan.planes_bytes,), 0x5A, dtype=torch.uint8, device=DEV)
        s = torch.zeros(plan.n_slices, dtype=torch.float32, device=DEV)
        y = torch.zeros_like(x)
        y2 = torch.zeros_like(x)
        plan.encode(x, seeds, p, s, ws)
        plan.decode(p, seeds, s, y, ws)
        plan.decode(p, seeds, s, y2, ws, base=base)
        torch.cuda.synchronize()
        outs.append((p.cpu(), s.cpu(), y.cpu(), y2.cpu()))
        del x, base, ws, p, s, y, y2
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert torch.equal(a, b)


def test_small_launch_split_bit_identical():
    """Tiny / small slices on their side stream give the same bytes as on the
    caller's stream: a mixed set through the default two-stream schedule vs
    the single-stream schedule."""
    from openfl_amd.codec import EdenPlan
    numels = [300, 2000, 5000, 9000, 17000, 33000, 70000, 1 << 20, (1 << 21) + 99, 150]
    res = []
    for streams in (1, 2):
        plan = EdenPlan(numels, 8, streams=streams)
        g = torch.Generator(device=DEV).manual_seed(31)
        x = torch.empty(plan.arena_numel, device=DEV).normal_(0, 0.01, generator=g)
        seeds = torch.arange(1, len(numels) + 1, dtype=torch.int32, device=DEV)
        ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
        p = torch.zeros(plan.planes_bytes, dtype=torch.uint8, device=DEV)
        s = torch.zeros(plan.n_slices, dtype=torch.float32, device=DEV)
        y = torch.zeros_like(x)
        plan.encode(x, seeds, p, s, ws)
        plan.decode(p, seeds, s, y, ws)
        torch.cuda.synchronize()
        res.append((p.cpu(), s.cpu(), y.cpu()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_plugin_call_contexts_identical(monkeypatch):
    """Small one-tensor calls go through cached per-shape call contexts
    (eden_pipeline._CallCtx): bytes, scales, seeds and decoded values equal
    the uncached path's, including repeated and interleaved shapes -- with
    the zero-copy mapped calls (slices <= 2^15) and with DMA copies."""
    from openfl_amd.pipelines import eden_pipeline as E
    sizes = [101, 777, 2048, 2049, 40000, 1 << 16, 777, 101, 32768, 32769, 5000]
    rng = np.random.default_rng(5)
    xs = [rng.standard_normal(n).astype(np.float32) for n in sizes]

    def run(use, mapped):
        monkeypatch.setattr(E, "_USE_CTX", use)
        monkeypatch.setattr(E, "_USE_MAPPED", mapped)
        pipe = E.EdenPipeline(n_bits=8, device=DEV)
        np.random.seed(11)
        enc = [pipe.forward(x) for x in xs]
        dec = [pipe.backward(d, [dict(m[0])]) for d, m in enc]
        return enc, dec

    (e0, d0) = run(False, False)
    for use, mapped in ((True, True), (True, False)):
        e1, d1 = run(use, mapped)
        for (b1, m1), (b0, m0), y1, y0 in zip(e1, e0, d1, d0):
            assert b1 == b0 and m1 == m0
            np.testing.assert_array_equal(y1, y0)


def test_plugin_pageable_path_identical(monkeypatch):
    """Larger one-tensor calls: x / planes straight from the caller's arrays
    (OFL_PLUGIN_PAGEABLE=1, ofl_eden_*_host_x) give the same bytes, seeds and
    decoded values as the default pinned-staging path."""
    from openfl_amd.pipelines import eden_pipeline as E
    sizes = [70000, 1 << 20, (1 << 21) + 5, 70000]
    rng = np.random.default_rng(9)
    xs = [rng.standard_normal(n).astype(np.float32) for n in sizes]

    def run(pageable):
        monkeypatch.setattr(E, "_PAGEABLE", pageable)
        pipe = E.EdenPipeline(n_bits=8, device=DEV)
        np.random.seed(13)
        enc = [pipe.forward(x) for x in xs]
        dec = [pipe.backward(d, [dict(m[0])]) for d, m in enc]
        return enc, dec

    (e1, d1), (e0, d0) = run(True), run(False)
    for (b1, m1), (b0, m0), y1, y0 in zip(e1, e0, d1, d0):
        assert b1 == b0 and m1 == m0
        np.testing.assert_array_equal(y1, y0)


@pytest.mark.parametrize("nbits", [1, 4, 8])
def test_small_set_bit_identical(nbits):
    """All tiny / small slices in one small-set launch (sset=1: 2^(15-P)
    slices of 2^P per 1024-thread workgroup, 4 tiny slices of one p, padding
    sub-blocks that store nothing) vs one launch per size class (sset=0):
    planes, scales, decoded values and the fused apply_delta are identical."""
    from openfl_amd.codec import EdenPlan
    rng = np.random.default_rng(nbits)
    numels = ([int(v) for v in rng.integers(9, 1024, 23)] + [2048] * 17 + [3000, 4096, 4100] * 3 + [8192] * 3 +
              [9000, 16384, 16385, 20000] + [32768] * 3 + [1 << 16, (1 << 17) + 7])
    rng.shuffle(numels)
    outs = []
    for sset in (0, 1):
        plan = EdenPlan(numels, nbits, sset=sset)
        g = torch.Generator(device=DEV).manual_seed(5)
        x = torch.empty(plan.arena_numel, device=DEV).normal_(0, 0.05, generator=g)
        base = torch.empty(plan.arena_numel, device=DEV).normal_(0, 1.0, generator=g)
        seeds = torch.arange(3, 3 + len(numels), dtype=torch.int32, device=DEV)
        ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
        p = torch.zeros(plan.planes_bytes, dtype=torch.uint8, device=DEV)
        s = torch.zeros(plan.n_slices, dtype=torch.float32, device=DEV)
        y = torch.zeros_like(x)
        y2 = torch.zeros_like(x)
        plan.encode(x, seeds, p, s, ws)
        plan.decode(p, seeds, s, y, ws)
        plan.decode(p, seeds, s, y2, ws, base=base)
        torch.cuda.synchronize()
        outs.append((p.cpu(), s.cpu(), y.cpu(), y2.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_concurrent_plugin_calls():
    """Concurrent per-tensor forward / backward calls (the gRPC pool's threads,
    aggregator_server.py:305): each caller gets exactly the bytes, metadata and
    values the serial per-tensor path gives for its seed, and the seeds use
    the np.random draws of the calls (one per call, as the reference)."""
    from openfl_amd.pipelines import EdenPipeline
    from openfl_amd.pipelines.eden_pipeline import _serial_sum
    pipe = EdenPipeline(n_bits=8, device=DEV)
    tr = pipe.transformers[0]
    rng = np.random.default_rng(29)
    xs = [(rng.standard_normal(int(n)) * 0.01).astype(np.float32) for n in rng.integers(200, 300_000, 48)]
    np.random.seed(5)
    fwd = [None] * len(xs)

    def enc(i):
        fwd[i] = pipe.forward(xs[i])
    th = [threading.Thread(target=lambda k=k: [enc(i) for i in range(k, len(xs), 8)]) for k in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    draws = sorted(np.random.RandomState(5).randint(1, 2 ** 16, size=len(xs)).tolist())
    got = []
    for x, (payload, mds) in zip(xs, fwd):
        md = mds[0]["int_to_float"]
        seed = int(md[0])
        got.append((seed - hash(_serial_sum(x) * 13 + 7)) % (2 ** 16))
        planes, scales, dims, total = tr.eden.compress(x, seed)
        assert payload == planes.tobytes()
        assert [md[2 + 2 * k] for k in range(len(dims))] == list(scales)
    assert sorted(got) == [d % (2 ** 16) for d in draws]
    dec = [None] * len(xs)

    def de(i):
        dec[i] = pipe.backward(fwd[i][0], [dict(m) for m in fwd[i][1]])
    th = [threading.Thread(target=lambda k=k: [de(i) for i in range(k, len(xs), 8)]) for k in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i, x in enumerate(xs):
        md = fwd[i][1][0]["int_to_float"]
        ref = tr.eden.decompress(np.frombuffer(fwd[i][0], np.uint8), md)
        np.testing.assert_array_equal(dec[i], ref.reshape(x.shape))


def test_wavg_encode_split_bit_identical():
    """The fused round-end encode (ofl_eden_encode_wavg: x = the weighted-
    average delta computed in the first row pass) over a 5-pass slice split
    into MALL sub-waves (64 MiB waves: the row-A sub-waves take explicit tile
    lists, unpaired in this kernel) gives the same planes and scales as the
    whole-slice schedule."""
    import ctypes
    from openfl_amd import _lib
    from openfl_amd.codec import EdenPlan
    numels = [(1 << 26) + 777, 3000, (1 << 20) + 5]
    g = torch.Generator(device=DEV).manual_seed(41)
    L = _lib.lib()
    outs = []
    for wave in (4096, 64):
        plan = EdenPlan(numels, 8, wave_mib=wave, streams=2)
        if not outs:
            xs = [torch.empty(plan.arena_numel, device=DEV).normal_(0, 0.01, generator=g) for _ in range(2)]
            base = torch.empty(plan.arena_numel, device=DEV).normal_(0, 0.1, generator=g)
            delta = torch.empty(plan.arena_numel, device=DEV).normal_(0, 0.01, generator=g)
        ptrs = torch.tensor([x.data_ptr() for x in xs], dtype=torch.int64, device=DEV)
        w = torch.tensor([0.3, 0.7], dtype=torch.float64, device=DEV)
        seeds = torch.tensor([11, 12, 13], dtype=torch.int32, device=DEV)
        ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=DEV)
        p = torch.full((plan.planes_bytes,), 0x5A, dtype=torch.uint8, device=DEV)
        s = torch.zeros(plan.n_slices, dtype=torch.float32, device=DEV)
        _lib.check(L.ofl_eden_encode_wavg(plan.handle, ptrs.data_ptr(), w.data_ptr(), 2, ctypes.c_double(1.0),
                                          base.data_ptr(), delta.data_ptr(), seeds.data_ptr(), p.data_ptr(),
                                          s.data_ptr(), ws.data_ptr(), ws.numel(), None))
        torch.cuda.synchronize()
        outs.append((p.cpu(), s.cpu()))
        del ws, p, s
    for a, b in zip(*outs):
        assert torch.equal(a, b)
