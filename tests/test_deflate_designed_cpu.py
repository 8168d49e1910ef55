"""The designed deflate cases (tests/deflate_cases.py) against zlib, on the
CPU: every valid stream is what its token list says (expand) and what zlib
reads; every invalid one makes zlib raise; the host member inflate
(lossy.gunzip -> ofl_gunzip_members) gives the same verdict and bytes; and the
reader used to inspect the device encoder's output (read_member) returns the
tokens the writer wrote.  The device tests run the same tables."""
import gzip
import zlib

import numpy as np
import pytest

from openfl_amd import _lib, lossy
from tests import deflate_cases as dc
from tests.deflate_writer import (END, Deflate, Raw, canonical, complete_by_zlib, expand, kraft_left, limited_lengths,
                                  read_member, tlz_member)

ERRORS = (zlib.error, EOFError, OSError)


@pytest.mark.parametrize("case", dc.valid_cases(), ids=lambda c: c.name)
def test_valid_case_is_what_zlib_reads(case):
    for m in case.members:
        assert expand(m.tokens) == m.data
        assert zlib.decompress(m.body, -15) == m.data
    assert gzip.decompress(case.stream) == case.data
    assert lossy.gunzip(case.stream, 4).tobytes() == case.data


@pytest.mark.parametrize("case", dc.invalid_cases(), ids=lambda c: c.name)
def test_invalid_case_is_refused_by_zlib(case):
    with pytest.raises(ERRORS):
        gzip.decompress(case.stream)
    with pytest.raises(_lib.CodecError):
        lossy.gunzip(case.stream, 4)
    assert gzip.decompress(case.twin) == case.twin_data
    assert lossy.gunzip(case.twin, 4).tobytes() == case.twin_data


@pytest.mark.parametrize("case", dc.tlz_cases(), ids=lambda c: c.name)
def test_tlz_case_is_valid_deflate(case):
    """Accepted or refused by the TLZ decoder, every TLZ case is valid deflate."""
    stream = b"".join(m.z for m in case.members)
    data = b"".join(m.data for m in case.members)
    for m in case.members:
        assert expand(m.tokens) == m.data and len(m.data) % 4 == 0
        assert zlib.decompress(m.body, -15) == m.data
    assert gzip.decompress(stream) == data
    assert lossy.gunzip(stream, 4).tobytes() == data


def _dynamic_only(case):
    return case.name != "fixed_block"


@pytest.mark.parametrize("case", [c for c in dc.tlz_cases() if _dynamic_only(c)], ids=lambda c: c.name)
def test_read_member_returns_what_tlz_member_wrote(case):
    stream, off = b"".join(m.z for m in case.members), 0
    for m in case.members:
        r = read_member(stream, off)                    # each member where it lies in the stream
        assert r["data_off"] == off + 28 + 4 * len(m.segbits)
        assert (r["kind"], r["version"], r["seglog"], r["size"]) == ("OZ", 1, 11, len(m.z))
        assert r["nval"] == len(m.data) // 4 and r["isize"] == len(m.data) and r["crc"] == zlib.crc32(m.data)
        assert r["segbits"] == m.segbits and r["nseg"] == len(m.segbits)
        toks = [t for b in r["blocks"] for _, t in b["tokens"]]
        want = list(m.tokens)
        if len(r["blocks"]) == 2:                       # the split block carries one more EOB
            cut = len(r["blocks"][0]["tokens"]) - 1
            want = want[:cut] + [END] + want[cut:]
        assert toks == [tuple(t) if isinstance(t, tuple) else t for t in want]
        assert (r["end_bit"] + 7) // 8 == r["data_len"] == len(m.body)
        bits = {at for b in r["blocks"] for at, _ in b["tokens"]}
        assert set(m.segbits) <= bits
        off += len(m.z)


def test_read_member_on_generic_members_and_its_refusals():
    by = {c.name: c for c in dc.valid_cases()}
    m = by["dyn_hclen_19_hlit_286_hdist_30"].members[0]
    r = read_member(m.z)
    b = r["blocks"][0]
    assert r["kind"] == "BC" and len(b["lit_lens"]) == 286 and len(b["dist_lens"]) == 30 and b["cl_lens"][15] > 0
    assert b["lit_lens"] == dc.LIT_1_15 and [t for _, t in b["tokens"]] == m.tokens
    m = by["dyn_repeat_codes"].members[0]
    b = read_member(m.z)["blocks"][0]
    assert b["lit_lens"] == dc.REPEAT_LIT and b["dist_lens"] == dc.REPEAT_DIST
    assert [t for _, t in b["tokens"]] == m.tokens
    b = read_member(by["dyn_hclen_5_hlit_257_hdist_1"].members[0].z)["blocks"][0]
    assert len(b["lit_lens"]) == 257 and b["dist_lens"] == [0] and sum(1 for x in b["cl_lens"] if x) == 2
    for name in ("stored_64", "fixed_all_literals"):
        with pytest.raises(ValueError):
            read_member(by[name].members[0].z)


# ---- the writer's own checks -------------------------------------------------------
def test_canonical_codes_match_rfc_1951_example():
    # RFC 1951 3.2.2: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> 010 011 100 101 110 00 1110 1111
    assert canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [0b010, 0b011, 0b100, 0b101, 0b110, 0b00, 0b1110, 0b1111]


def test_bit_writer_order():
    w = Deflate()
    w.bits(0b1, 1)
    w.bits(0b01, 2)
    w.code(0b110, 3)          # Huffman codes go most significant bit first
    w.bits(0b10, 2)
    assert w.getvalue() == bytes([0b10_011_01_1])
    w.align()
    w.raw_bytes(b"\xAA")
    assert w.getvalue() == bytes([0b10011011, 0xAA]) and w.bitpos == 16


@pytest.mark.parametrize("maxlen", [7, 10, 11, 15])
def test_limited_lengths_complete_and_bounded(maxlen):
    rng = np.random.default_rng(maxlen)
    for trial in range(30):
        n = int(rng.integers(2, min(286, 1 << maxlen)))
        freq = [int(f) for f in (rng.integers(0, 3, n) * (2.0 ** rng.integers(0, 24, n))).astype(np.int64)]
        lens = limited_lengths(freq, maxlen)
        used = [s for s in range(n) if freq[s]]
        if not used:
            assert not any(lens)
            continue
        assert kraft_left(lens) == 0 and max(lens) <= maxlen
        assert all(lens[s] for s in used)
        if len(used) > 1:
            assert all(lens[s] == 0 for s in range(n) if not freq[s])
    # a steep distribution needs the limit: unlimited, the rarest symbols sit 20 deep
    steep = [1 << (20 - min(k, 20)) for k in range(22)]
    assert max(limited_lengths(steep, 15)) == 15 and max(limited_lengths(steep, 11)) == 11


def test_complete_by_zlib_is_zlibs_rule():
    """inf_build's completeness rule, as the tests state it, checked against zlib itself on
    hand-written dynamic blocks: incomplete sets are refused, except a set
    whose longest code is 1 bit, and never the code-length alphabet."""
    def accepts(lit, dist, tokens, **kw):
        body = Deflate().dynamic(tokens, lit, dist, True, **kw).getvalue()
        try:
            zlib.decompress(body, -15)
            return True
        except zlib.error:
            return False
    a = [0] * 257
    a[97], a[256] = 2, 1
    assert not complete_by_zlib(a) and not accepts(a, [0], [97, END])
    one = [0] * 257
    one[256] = 1
    assert complete_by_zlib(one) and accepts(one, [0], [END])
    lit = [0] * 258
    lit[97] = lit[256] = 2
    lit[257] = 1
    assert complete_by_zlib(lit)
    assert not complete_by_zlib([2, 2]) and not accepts(lit, [2, 2], [97, (3, 1), END])
    assert complete_by_zlib([1]) and accepts(lit, [1], [97, (3, 1), END])
    assert complete_by_zlib([0]) and accepts(lit, [0], [97, END])
    hole = [0] * 19
    hole[0], hole[8] = 1, 2
    assert not complete_by_zlib(hole, is_cl=True) and not accepts(dc.LIT_ALL8, [0], [5, END], cl_lens=hole)
    lone = [0] * 19
    lone[0] = 1
    assert not complete_by_zlib(lone, is_cl=True)


def test_case_tables_cover_what_they_claim():
    names = {c.name for c in dc.valid_cases()}
    assert {f"dyn_eob15_end{r}" for r in range(8)} <= names
    new = [c.name for c in dc.invalid_cases() if c.new]
    assert sorted(new) == sorted(f"incomplete_{k}_{u}" for k in ("literals", "distances", "cl") for u in ("used", "unused"))
    acc = [c for c in dc.tlz_cases() if c.accepted]
    assert len(acc) >= 18 and len(dc.tlz_cases()) - len(acc) >= 11
    for name, want in (("misaligned_12", 12), ("misaligned_4", 4), ("misaligned_8", 8)):
        ms = next(f for k, f in dc.MISALIGNED.items() if k.startswith(name))()
        # the middle member: several segments of many ops each, starting `want` bytes past a multiple of 16
        assert len(ms[0].data) % 16 == want and len(ms[1].segbits) >= 2
        assert sum(1 for t in ms[1].tokens if isinstance(t, tuple)) >= 16
    m = dc.seven_segments()
    assert len(m.segbits) == 7 and len(m.data) == 4 * 14336
    lad = {c.name: c for c in dc.tlz_cases()}
    for name, lmax, dmax in (("code_lengths_11_and_10", 11, 10), ("literal_code_length_12", 12, 10),
                             ("distance_code_length_11", 11, 11)):
        b = read_member(lad[name].members[0].z)["blocks"][0]
        assert (max(b["lit_lens"]), max(b["dist_lens"])) == (lmax, dmax)
    assert isinstance(Raw(1, 1), tuple) and tlz_member([[("lit", 3)]]).data == np.float32([3]).tobytes()
