"""GPU: lossy.gunzip_lut_batch (k_tlz_small, and k_tlz_ops / k_tlz_resolve over
one member table), RoundEnd.ingest on it, the lossy pipelines' backward_batch.
The reference is the host's: gzip.decompress of the payload as float32, then
the sequential key -> value replacement (kc_pipeline.py:79-83) in NumPy; equal
float32 bits.  Payloads: lossy.gzip_ranks of designed ranks at the sizes where
the decoder changes path: 2048 the last one-segment member, 2049 the first of
two segments, 131072 a full member, 131073 a full and a one-segment member."""
import ctypes
import functools
import gzip

import numpy as np
import pytest
import torch

from tests import bgzf
from tests.round_stream_cases import DEV, F, bits, make_pipeline, tensors

pytestmark = pytest.mark.gpu
SIZES = (6, 7, 63, 64, 65, 2047, 2048, 2049, 4096, 131072, 131073, 131072 + 2049)
SENTINEL = 123.25


def _ranks(content, n, t):
    if content == "one":
        return np.full(n, t % 32, F)
    if content == "cycle":
        return (np.arange(n) % 32).astype(F)
    # runs: a period of the full window (copies of 64 values at distance 8192) and one long run of a rank
    x = np.tile(np.random.default_rng(t).integers(0, 32, 8192), n // 8192 + 1)[:n].astype(F)
    x[n // 8:n // 2] = 7
    return x


def _map(t):
    """Per tensor another map: all 32 keys; fewer keys than ranks (the others
    stay); a value equal to a later key (replaced again); neighbours differ."""
    kind = t % 3
    if kind == 0:
        return {k: float(F(0.001 * (k + 1) * (t + 1))) for k in range(32)}
    if kind == 1:
        return {0: -0.5 - t, 1: 0.25 + t}
    return {0: 5.0, 7: float(t), 5: -1.5, 31: 2.0}


@functools.lru_cache(maxsize=None)
def _payloads(content):
    from openfl_amd import lossy
    return [lossy.gzip_ranks(torch.from_numpy(_ranks(content, n, t)).to(DEV)) for t, n in enumerate(SIZES)]


def _reference(payload, m):
    data = np.frombuffer(gzip.decompress(payload), F).copy()
    for key in (m or {}):
        data[data == F(key)] = F(m[key])
    return data


def _layout(sizes, reverse, misalign):
    """Element offsets with a gap after every tensor; misalign: offsets 1, 2, 3
    mod 4 in turn (4- but not 16-byte aligned outputs), else multiples of 4."""
    order = list(range(len(sizes)))[::-1] if reverse else list(range(len(sizes)))
    offsets, at = [0] * len(sizes), 0
    for j, t in enumerate(order):
        offsets[t] = at + (1 + j % 3 if misalign else 0)
        at = (offsets[t] + sizes[t] + 3) // 4 * 4 + 4
    return offsets, at


def _decode_and_check(payloads, sizes, maps, offsets, total):
    from openfl_amd import lossy
    arena = torch.full((total,), SENTINEL, dtype=torch.float32, device=DEV)
    assert lossy.gunzip_lut_batch(payloads, offsets, sizes, maps, arena) is arena
    got = arena.cpu().numpy()
    untouched = np.ones(total, bool)
    for t, n in enumerate(sizes):
        want = _reference(payloads[t], maps[t] if maps is not None else None)
        assert want.size == n and bits(got[offsets[t]:offsets[t] + n]) == bits(want), (t, n)
        untouched[offsets[t]:offsets[t] + n] = False
    assert bits(got[untouched]) == bits(np.full(int(untouched.sum()), SENTINEL, F))


@pytest.mark.parametrize("content", ["one", "cycle", "runs"])
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
def test_edge_sizes(reverse, misalign, content):
    """Right values, and from the batch: one launch of each kernel, no tensor on the one-stream path."""
    from openfl_amd import _lib
    offsets, total = _layout(SIZES, reverse, misalign)
    payloads = _payloads(content)
    L = _lib.lib()
    L.ofl_gzip_profile(1)
    try:
        _decode_and_check(payloads, list(SIZES), [_map(t) for t in range(len(SIZES))], offsets, total)
        names, ms, ln, nk = ctypes.create_string_buffer(4096), np.zeros(16), np.zeros(16, np.int64), ctypes.c_int()
        _lib.check_gzip(L.ofl_gzip_profile_collect(names, 4096, ms.ctypes.data, ln.ctypes.data, 16, ctypes.byref(nk)))
    finally:
        L.ofl_gzip_profile(0)
    assert dict(zip(names.value.decode().split("\n")[:nk.value], ln.tolist())) == {
        "tlz::k_tlz_ops": 1, "tlz::k_tlz_resolve": 1, "tlz::k_tlz_small": 1}


@pytest.mark.parametrize("lut", [True, False], ids=["lut", "ranks"])
def test_mixed_upload(lut):
    """A stock gzip.compress payload and a BGZF one among TLZ payloads: the
    table leaves them out and they decode alone, into the same arena."""
    tlz = _payloads("runs")
    raw = [_ranks("cycle", 300, 0).tobytes(), _ranks("runs", 20000, 1).tobytes()]
    payloads = [tlz[6], gzip.compress(raw[0]), tlz[8], bgzf.member_indexed(raw[1]), tlz[3], tlz[10]]
    sizes = [SIZES[6], 300, SIZES[8], 20000, SIZES[3], SIZES[10]]
    offsets, total = _layout(sizes, False, True)
    _decode_and_check(payloads, sizes, [_map(t) for t in range(len(sizes))] if lut else None, offsets, total)


SHAPES = [(1,), (6,), (7, 9), (2048,), (2049,), (3, 1400), (131073,)]


@functools.lru_cache(maxsize=None)
def _round(name):
    """(RoundEnd, its upload [(payload, metadata list)], shared and never modified)."""
    from openfl_amd.aggregation import RoundEnd
    re = RoundEnd(make_pipeline(name), SHAPES, device=DEV)
    np.random.seed(5)
    return re, [re.pipeline.forward(x) for x in tensors(SHAPES, 31)]


@pytest.mark.parametrize("delta", [True, False], ids=["delta", "nodelta"])
@pytest.mark.parametrize("name", ["kc", "skc", "stc"])
def test_ingest_and_backward_batch_equal_backward(name, delta):
    re, items = _round(name)
    want = [np.asarray(re.pipeline.backward(p, list(mds)), F) for p, mds in items]
    before = [[dict(md) for md in mds] for _, mds in items]
    batch = re.pipeline.backward_batch(items)
    assert [[dict(md) for md in mds] for _, mds in items] == before    # the metadata lists stay
    for y, w in zip(batch, want):
        assert y.dtype == F and y.shape == w.shape and bits(y) == bits(w)
    base_h = tensors(SHAPES, 3, 0.1)
    got = re.ingest(items, delta=delta, base_arena=re.pack(base_h) if delta else None).cpu().numpy()
    for i, w in enumerate(want):
        w = base_h[i] + w if delta else w
        assert bits(got[re.offsets[i]:re.offsets[i] + re.numels[i]]) == bits(w.reshape(-1)), i


@pytest.mark.parametrize("at", [-8, -4], ids=["crc", "isize"])
@pytest.mark.parametrize("tensor", [3, 4], ids=["small_member", "large_member"])
def test_bad_trailer_names_the_tensor_and_leaves_out(tensor, at):
    """A flipped CRC-32 or ISIZE byte of a one-segment and of a two-segment
    member: the decode itself is unchanged, the comparison fails."""
    from openfl_amd._lib import CodecError
    re, items = _round("kc")
    bad = bytearray(items[tensor][0])
    bad[len(bad) + at] ^= 4
    items = [(bytes(bad), mds) if i == tensor else (p, mds) for i, (p, mds) in enumerate(items)]
    out = torch.full((re.arena_numel,), SENTINEL, dtype=torch.float32, device=DEV)
    with pytest.raises(CodecError, match=f"tensor {tensor}:"):
        re.ingest(items, delta=False, out=out)
    assert bits(out.cpu().numpy()) == bits(np.full(re.arena_numel, SENTINEL, F))
