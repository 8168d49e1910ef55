"""The TLZ decoder and encoder without the fallback that hides them.

lossy.gunzip_device hands every member the TLZ decoder refuses to the generic
inflate, which decodes it: a decoder that wrongly refuses, or an encoder that
writes what the decoder refuses, only costs time there.  Here the decoder's
own verdict is read (ofl_inflate_tlz_async + ofl_inflate_tlz_check) on
designed members (tests/deflate_cases.py: accepted ones must be accepted and
equal zlib; valid deflate that is not TLZ must be refused and still decode
through the fallback), and what lossy.gzip_ranks writes is read back symbol by
symbol with tests/deflate_writer.py's reader, not with our decoder."""
import gzip
import heapq
import zlib

import numpy as np
import pytest

from tests import deflate_cases as dc
from tests import deflate_device as dev
from tests.deflate_writer import END, LBASE, complete_by_zlib, expand, read_member

pytestmark = pytest.mark.gpu
DEV = dev.DEV
SEG_BYTES = 4 * 2048


@pytest.mark.parametrize("case", dc.tlz_cases(), ids=lambda c: c.name)
def test_tlz_decoder_verdict(case):
    z = b"".join(m.z for m in case.members)
    want = gzip.decompress(z)
    assert want == b"".join(m.data for m in case.members)
    verdict, got = dev.tlz_decode(z)
    assert verdict == ("accepted" if case.accepted else "refused")
    if case.accepted:
        assert got == want
    assert dev.gunzip_device(z, len(want)) == want            # refused members: through the fallback


def test_fused_lut_on_the_seven_segment_member():
    """ofl_inflate_tlz_launch_lut on a member the decoder accepts (the verdict
    table above): tensor boundaries inside one thread's 8 values, six tensors
    inside one segment (more than the LDS slots: the lut_find path), gaps that
    keep the rank, a tensor over several segments, one ending with the member."""
    import torch
    from openfl_amd import lossy
    from oracle import kc
    m = dc.seven_segments()
    ranks = np.frombuffer(zlib.decompress(m.body, -15), np.float32)
    spans = [(3, 2), (6, 9), (2050, 5), (2060, 3), (2070, 100), (2200, 7), (2300, 11), (2400, 50), (4000, 5000),
             (10239, 3), (14000, 336)]
    rng = np.random.default_rng(5)
    maps = []
    for t in range(len(spans)):
        mp = {float(r): float(np.float32(rng.standard_normal())) for r in range(32)}
        if t % 2 == 0:
            mp[0.0] = 2.0                                     # 0 -> 2 -> mp[2]: the sequential chain
        maps.append(mp)
    want = ranks.copy()
    for (o, n), mp in zip(spans, maps):
        want[o:o + n] = kc.lut_sequential(ranks[o:o + n].copy(), mp)
    offs, nums = [o for o, _ in spans], [n for _, n in spans]
    out = torch.full((ranks.size + 16,), -7.0, dtype=torch.float32, device=DEV)
    got = lossy.gunzip_device(m.z, out.view(torch.uint8), lut=lossy.lut_tables(offs, nums, maps, DEV))
    np.testing.assert_array_equal(got.view(torch.float32).cpu().numpy(), want)
    assert float(out[ranks.size:].min()) == float(out[ranks.size:].max()) == -7.0


@pytest.mark.parametrize("name", list(dc.MISALIGNED), ids=str)
def test_fused_lut_on_misaligned_members(name):
    """The fused LUT on streams whose multi-segment members start 4, 8 or 12
    bytes past a multiple of 16 (accepted in the verdict table above): the
    resolve's scalar value store, with tensors over the member boundaries."""
    import torch
    from openfl_amd import lossy
    from oracle import kc
    members = dc.MISALIGNED[name]()
    z = b"".join(m.z for m in members)
    ranks = np.frombuffer(gzip.decompress(z), np.float32)
    n = ranks.size
    spans = [(0, 2), (2, 9), (13, 1000), (1500, 7), (2040, n - 2040 - 3)]
    rng = np.random.default_rng(len(name))
    maps = [{float(r): float(np.float32(rng.standard_normal())) for r in range(32)} for _ in spans]
    maps[2][0.0] = 2.0
    want = ranks.copy()
    for (o, k), mp in zip(spans, maps):
        want[o:o + k] = kc.lut_sequential(ranks[o:o + k].copy(), mp)
    out = torch.full((n + 16,), -7.0, dtype=torch.float32, device=DEV)
    got = lossy.gunzip_device(z, out.view(torch.uint8), lut=lossy.lut_tables([o for o, _ in spans], [k for _, k in spans],
                                                                             maps, DEV))
    np.testing.assert_array_equal(got.view(torch.float32).cpu().numpy(), want)
    assert float(out[n:].min()) == float(out[n:].max()) == -7.0


# ---- the encoder ------------------------------------------------------------------
def _inputs():
    rng = np.random.default_rng(2024)
    kc6 = [0.07, 0.2, 0.23, 0.23, 0.2, 0.07]
    geo = 0.5 ** np.arange(32)
    block = rng.integers(0, 32, 8193)
    x = {
        "constant": np.full(5000, 2.0),
        "one": np.array([5.0]),
        "period2": np.tile([1.0, 4.0], 5000),
        "period3": np.tile([3.0, 0.0, 7.0], 3334),
        "repeat_8192": np.tile(block[:8192], 3),
        "repeat_8193": np.tile(block, 3),
        "all32": rng.integers(0, 32, 20000),
        "runs": np.repeat(rng.integers(0, 6, 501), 100)[:50000],
        "geometric": rng.choice(32, 65536, p=geo / geo.sum()),
    }
    for n in (2047, 2048, 2049, 131071, 131072, 131073):
        x[f"n{n}"] = rng.choice(6, n, p=kc6)
    return {k: np.asarray(v, np.float32) for k, v in x.items()}


INPUTS = _inputs()
# every lit/len symbol a valid rank stream can use: the 26 distinct bytes of
# float32(0..31), end of block, and the 18 length codes that hold a multiple
# of 4 bytes in 12..256 (265, 267, 269..284): 45 in all, so huff_lengths_wave's
# serial fallback (more than 64 used symbols) is out of reach of valid ranks
# (distances: 30 symbols at the most; code lengths: 19)
MAX_LITLEN_SYMBOLS = 45
assert len({b for r in range(32) for b in np.float32(r).tobytes()}) == 26


def huffman_depth(freq):
    """Depth of the deepest leaf of an unconstrained Huffman tree."""
    heap = [(f, 0) for f in freq if f]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def check_member(r, raw):
    """One member of the encoder's stream, as read by read_member, against
    the bytes it must hold."""
    assert len(r["blocks"]) == 1 and r["blocks"][0]["bfinal"] == 1           # one final dynamic block
    b = r["blocks"][0]
    assert (r["kind"], r["version"], r["seglog"]) == ("OZ", 1, 11)
    assert r["nval"] == len(raw) // 4 and r["isize"] == len(raw) and r["crc"] == zlib.crc32(raw)
    assert r["nseg"] == len(r["segbits"]) == -(-len(raw) // SEG_BYTES)
    assert (r["end_bit"] + 7) // 8 == r["data_len"]                            # the size field: data ends with the block
    assert max(b["lit_lens"]) <= 11 and max(b["dist_lens"] + [0]) <= 10 and max(b["cl_lens"]) <= 7
    assert complete_by_zlib(b["lit_lens"]) and complete_by_zlib(b["dist_lens"]) and complete_by_zlib(b["cl_lens"], True)
    pos, starts, tokens = 0, {}, []
    for at, t in b["tokens"]:
        starts.setdefault(pos, at)
        tokens.append(t)
        if t == END:
            break
        if isinstance(t, int):
            pos += 1
            continue
        ln, d = t
        assert ln % 4 == 0 and 12 <= ln <= 256, t                              # 3..64 whole values
        assert d % 4 == 0 and 4 <= d <= 32768 and d <= pos, (t, pos)           # 1..8192 whole values, inside the member
        assert pos % 4 == 0 and pos // SEG_BYTES == (pos + ln - 1) // SEG_BYTES, (t, pos)   # no segment end crossed
        pos += ln
    assert pos == len(raw) and expand(tokens) == raw
    assert r["segbits"] == [starts[s * SEG_BYTES] for s in range(r["nseg"])]
    return b, tokens


@pytest.mark.parametrize("name", list(INPUTS), ids=str)
def test_encoder_output_read_without_our_decoder(name):
    import torch
    from openfl_amd import lossy
    x = INPUTS[name]
    raw = x.tobytes()
    z = lossy.gzip_ranks(torch.from_numpy(x).to(DEV))
    assert gzip.decompress(z) == raw
    # the TLZ decoder itself takes the stream (through gunzip_device a refusal
    # would only cost time); first, so that an encoder writing what the
    # decoder refuses is reported as that
    verdict, got = dev.tlz_decode(z)
    assert verdict == "accepted" and got == raw
    off, done, depths, nsym = 0, 0, [], 0
    while off < len(z):
        r = read_member(z, off)
        part = raw[done:done + r["isize"]]
        assert r["isize"] == min(4 * 131072, len(raw) - done)                   # members of 131072 values
        b, tokens = check_member(r, part)
        freq = [0] * 286
        for t in tokens:
            freq[256 if t == END else t if isinstance(t, int) else 257 + max(
                i for i in range(29) if LBASE[i] <= t[0])] += 1
        used = sum(1 for f in freq if f)
        # (a lone symbol's partner has a code without being used: one more)
        assert used <= sum(1 for ln in b["lit_lens"] if ln) <= used + 1
        nsym = max(nsym, used)
        depths.append(huffman_depth(freq))
        off += r["size"]
        done += r["isize"]
    assert off == len(z) and done == len(raw)
    print(f"{name}: members {len(depths)}, lit/len symbols used {nsym}, unconstrained Huffman depth {depths}")
    if name == "constant":
        # a lone distance symbol is written as a single 1-bit code (no partner):
        # incomplete, and allowed by inf_build's rule as by zlib's
        assert b["dist_lens"].count(1) == 1 and sum(b["dist_lens"]) == 1
    if name == "one":
        # no copy: HDIST is 1 at the least, and that one length is 0 or a lone
        # (unused) 1-bit code; zlib takes either (observed: [1])
        assert b["dist_lens"] in ([0], [1])
    assert nsym <= MAX_LITLEN_SYMBOLS
    if name == "geometric":
        # the condition of this case: without the limit the code would be deeper
        # than kLitMax = 11, so huff_lengths_wave's halving loop ran.  Observed
        # on an MI355X: 26 lit/len symbols used, unconstrained depth 14 (the
        # kc6 members of 131071 and 131073 values and repeat_8192 reach 12)
        assert max(depths) > 11, depths
