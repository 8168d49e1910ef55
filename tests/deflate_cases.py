"""The designed deflate cases, as tables shared by the CPU checks
(test_deflate_designed_cpu.py), the device inflate tests
(test_gpu_inflate_designed.py, also run by its child processes under the
opt-in decoder variants) and the TLZ tests (test_gpu_tlz_designed.py).  Every
stream is written token by token with tests/deflate_writer.py.

A block with HCLEN 4 sends code-length lengths for 16, 17, 18 and 0 only, so
every literal length it can describe is 0 and it has no end-of-block code:
the smallest valid count is 5 (dyn_hclen_5_...), and HCLEN 4 is the second
"no EOB code" row of the invalid table."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from tests.deflate_writer import (DBASE, DEXT, END, FIXED_LIT, LEXT, Deflate, Raw, SymCopy, bc_member, canonical,
                                  dist_sym, expand, fitted_lengths, kraft_left, len_sym, tlz_member)

# a valid member: its bytes, the deflate data alone, the expected output and the flat token list
Member = namedtuple("Member", "z body data tokens")
# valid: stream + expected bytes; invalid: bad stream, its intact twin, the twin's bytes, the error text to match
Valid = namedtuple("Valid", "name members stream data")
Invalid = namedtuple("Invalid", "name stream twin twin_data match new")


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def rev(code, n):
    return int(format(code, f"0{n}b")[::-1], 2) if n else 0


class Mem:
    """One member, block by block, with the flat token list beside it (stored
    bytes count as literals) so that expand() gives the expected bytes."""

    def __init__(self):
        self.w = Deflate()
        self.toks = []

    def stored(self, data, final=False, **kw):
        self.w.stored(data, final, **kw)
        self.toks += list(data)
        return self

    def fixed(self, tokens, final=False, **kw):
        self.w.fixed(tokens, final, **kw)
        self.toks += tokens
        return self

    def dynamic(self, tokens, lit=None, dist=None, final=False, **kw):
        if lit is None or dist is None:
            fl, fd = fitted_lengths(tokens)
            lit, dist = (fl if lit is None else lit), (fd if dist is None else dist)
        self.w.dynamic(tokens, lit, dist, final, **kw)
        self.toks += tokens
        return self

    def done(self, data=None, **kw):
        body = self.w.getvalue()
        data = expand(self.toks) if data is None else data
        wide = 18 + len(body) + 8 > 65536
        return Member(bc_member(body, data, wide=wide, **kw), body, data, self.toks)


def lits(data):
    return list(data)


def small(seed=0):
    """A small fixed-block member that pads a case's stream to a few members."""
    return Mem().fixed(lits(noise(21 + seed, 900 + seed)) + [(5, 3), END], True).done()


def valid(name, *members, pad=True):
    ms = list(members) + ([small(len(name))] if pad else [])
    return Valid(name, ms, b"".join(m.z for m in ms), b"".join(m.data for m in ms))


# ---- code sets used by several cases -------------------------------------------
def lens_1_to_15(assign, n):
    """Lengths 1..14 once and 15 twice (complete) for the 16 symbols of
    `assign`, in that order."""
    assert len(assign) == 16
    out = [0] * n
    for k, s in enumerate(assign):
        out[s] = min(k + 1, 15)
    assert kraft_left(out) == 0
    return out


# literals A..I at 1..9 bits; literals 0, 200, 255 at 10..12; length code 260
# (6 bytes) at 13; EOB at 14; length code 285 (258 bytes) and literal 7 at 15
LIT_1_15 = lens_1_to_15([65, 66, 67, 68, 69, 70, 71, 72, 73, 0, 200, 255, 260, 256, 285, 7], 286)
# the same with EOB as one of the two 15-bit codes
LIT_EOB15 = lens_1_to_15([65, 66, 67, 68, 69, 70, 71, 72, 73, 0, 200, 255, 260, 7, 285, 256], 286)
DIST_1_15 = lens_1_to_15(list(range(16)), 16)


def unrle(header_syms):
    out = []
    for h in header_syms:
        if isinstance(h, int):
            out.append(h)
        elif h[0] == 16:
            out += [out[-1]] * h[1]
        else:
            out += [0] * h[1]
    return out


# every repeat code at both ends of its count, a 16 right after an 18, and a 16
# whose run of three covers the last literal length and the first two distance
# lengths: 263 literal/length lengths, then 9 distance lengths
REPEAT_HEADER = [(18, 138), (18, 11), (16, 3), (17, 10), (17, 3), 8, (16, 6), (16, 3), (18, 81),
                 1, 2, 3, 4, 6, 8, (16, 3), 7, 6, 5, 4, 3, 2, 1]
REPEAT_LENS = unrle(REPEAT_HEADER)
REPEAT_LIT, REPEAT_DIST = REPEAT_LENS[:263], REPEAT_LENS[263:]
assert len(REPEAT_LENS) == 272 and kraft_left(REPEAT_LIT) == 0 and kraft_left(REPEAT_DIST) == 0

# 256 codes of 8 bits (literals 1..255 and EOB): the only lengths are 0 and 8,
# so five code-length lengths (16, 17, 18, 0, 8) describe the block
LIT_ALL8 = [0] + [8] * 256
CL_0_8 = [1 if s in (0, 8) else 0 for s in range(19)]


def copy_case(length):
    """Every distance at which a copy of `length` takes another path: below,
    at and above the 64-lane width, the copy's own length (overlap or not),
    the last distance inside the 1 KiB ring (d + len == 1024), the first
    outside it, and the far end of the window."""
    toks = []
    for d in (1, 2, 3, 63, 64, 65, length, 1024 - length, 1025 - length, 32768):
        toks += [d & 0xFF, (length, d)]
    return Mem().stored(noise(32768, 40 + length)).dynamic(toks + [END], final=True).done()


@lru_cache(maxsize=None)
def valid_cases():
    c = []
    # ---- stored blocks
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 511, 513, 65535):
        c.append(valid(f"stored_{n}", Mem().stored(noise(n, n), True).done()))
    for r in range(8):
        # a fixed block of 3 + 8 a + 9 b + 7 bits: b nine-bit literals set its length mod 8
        m = Mem().fixed([1, 2, 3] + [200 + k for k in range((r - 2) % 8)] + [END])
        assert m.w.bitpos % 8 == r
        c.append(valid(f"stored_after_fixed_mod{r}", m.stored(noise(70, r), True).done()))
    c.append(valid("stored_empty_between_huffman",
                   Mem().fixed(lits(b"abcabc") + [(4, 3), END]).stored(b"").dynamic(lits(b"xyz") + [(9, 12), END],
                                                                                   final=True).done()))
    # ---- fixed blocks
    c.append(valid("fixed_all_literals", Mem().fixed(list(range(256)) + [END], True).done()))
    toks = lits(noise(300, 7))
    for ls in range(29):
        for lx in sorted({0, (1 << LEXT[ls]) - 1}):
            toks += [ls, SymCopy(257 + ls, lx, 5, 0)]      # distance 7
    c.append(valid("fixed_length_codes", Mem().fixed(toks + [END], True).done()))
    toks = []
    for ds in range(30):
        for dx in sorted({0, (1 << DEXT[ds]) - 1}):
            toks += [ds, SymCopy(259, 0, ds, dx)]          # 5 bytes
    c.append(valid("fixed_distance_codes", Mem().stored(noise(32768, 8)).fixed(toks + [END], True).done()))
    # ---- copy geometry
    for length in (3, 64, 65, 258):
        c.append(valid(f"copy_len{length}", copy_case(length)))
    c.append(valid("copy_reaches_first_byte",
                   Mem().fixed(lits(b"abcdef") + [(6, 6), END], True).done(),
                   Mem().fixed(lits(b"abcde") + [(258, 5), (70, 263), END], True).done()))
    c.append(valid("copy_of_global_readback",
                   Mem().stored(noise(2000, 9)).dynamic([(258, 1500), (258, 258), (100, 1200), (258, 800), 5,
                                                         (65, 1100), END], final=True).done()))
    # ---- dynamic blocks: code lengths
    toks = [65, 66, 67, 68, 69, 70, 71, 72, 73, 0, 200, 255, 7, (6, 2), (258, 1), 65, (6, 1), END]
    c.append(valid("dyn_lit_lengths_1_15", Mem().dynamic(toks, LIT_1_15, [1, 1], True).done()))
    toks = lits(noise(300, 10))
    for ds in range(16):
        toks += [(4, DBASE[ds]), ds, (9, DBASE[ds] + (1 << DEXT[ds]) - 1)]
    fl, _ = fitted_lengths(toks + [END])
    c.append(valid("dyn_dist_lengths_1_15", Mem().dynamic(toks + [END], fl, DIST_1_15, True).done()))
    # ---- dynamic blocks: header counts
    m = Mem().dynamic(lits(range(1, 256)) + [END], LIT_ALL8, [0], True, cl_lens=CL_0_8)
    c.append(valid("dyn_hclen_5_hlit_257_hdist_1", m.done()))   # (HCLEN 4 can describe no EOB code: see the invalid table)
    m = Mem().dynamic([65, 66, 7, (258, 1), (6, 1), END], LIT_1_15, [1] + [0] * 28 + [1], True)
    c.append(valid("dyn_hclen_19_hlit_286_hdist_30", m.done()))
    # ---- dynamic blocks: repeat codes
    toks = [165, 170, 174, (3, 1), (4, 2), (5, 3), (6, 4), (7, 5), (8, 7), (3, 9), (4, 13), (5, 17), END]
    c.append(valid("dyn_repeat_codes", Mem().dynamic(toks, REPEAT_LIT, REPEAT_DIST, True, header_syms=REPEAT_HEADER).done()))
    # ---- dynamic blocks: degenerate code sets
    c.append(valid("dyn_no_distance_codes", Mem().dynamic(lits(b"literals only, no copies") + [END], dist=[0], final=True).done()))
    c.append(valid("dyn_lone_distance_code", Mem().dynamic(lits(b"ab") + [(20, 1), 99, (3, 1), END], dist=[1], final=True).done()))
    c.append(valid("dyn_eob_alone", Mem().dynamic([END], [0] * 256 + [1], [0], True).done()))
    # ---- block ends: a 15-bit EOB ending at each bit of the last byte
    ends = set()
    for r in range(8):
        m = Mem().dynamic([66, 0, 7] + [65] * r + [END], LIT_EOB15, [1, 1], True)
        ends.add(m.w.bitpos % 8)
        c.append(valid(f"dyn_eob15_end{m.w.bitpos % 8}", m.done()))
    assert len(ends) == 8
    # ---- block structure
    first = noise(600, 11)
    c.append(valid("three_blocks_copy_into_first",
                   Mem().stored(first).fixed(lits(b"second block ") + [(13, 13), END]).dynamic(
                       lits(b"third") + [(258, 600 + 26 + 5), (30, 700), END], final=True).done()))
    # ---- ISIZE and alignment
    def sized(n, seed):
        toks = lits(noise(min(n, 40), seed))
        left = n - len(toks)
        while left:
            ln = min(left, 258)
            ln -= 3 if 0 < left - ln < 3 else 0
            toks.append((ln, 33))
            left -= ln
        return Mem().fixed(toks + [END], True).done()
    sizes = (0, 1, 15, 16, 17, 63, 64, 65, 1008, 1023, 1024, 1025, 4096)
    for n in sizes:
        c.append(valid(f"isize_{n}", sized(n, n), pad=False))
    c.append(valid("isize_misaligned_offsets", *[sized(n, 100 + n) for n in sizes], pad=False))
    c.append(valid("isize_aligned_offsets", *[sized(n, 200 + n) for n in (16, 1024, 64, 1008, 4096, 1024)], pad=False))
    assert len({v.name for v in c}) == len(c)
    for v in c:
        for m in v.members:
            assert expand(m.tokens) == m.data
    return c


# ---- invalid ---------------------------------------------------------------------
def fixed_raw(sym):
    """A fixed-block literal/length symbol as raw bits (286 and 287 have codes too)."""
    return Raw(rev(canonical(FIXED_LIT)[sym], FIXED_LIT[sym]), FIXED_LIT[sym])


SIZE = "differs from its ISIZE"


def pair(name, bad, good, match="corrupt deflate data", new=False):
    """bad / good: members (or raw member bytes) -> streams of three members,
    the middle one being the case.  match: the text of the device's error,
    which names the status flag the refusing check sets (kInfCorrupt: 'corrupt
    deflate data', kInfSize: 'differs from its ISIZE', kInfCrc: 'CRC'); a
    member refused before its end never reaches the CRC."""
    a, b = small(1), small(2)
    bz = bad if isinstance(bad, bytes) else bad.z
    return Invalid(name, a.z + bz + b.z, a.z + good.z + b.z, a.data + good.data + b.data, match, new)


@lru_cache(maxsize=None)
def invalid_cases():
    c = []
    base = lits(b"designed deflate ") + [(17, 17), 33, (9, 4)]
    text = expand(base)
    good = Mem().fixed(base + [END], True).done()
    gdyn = Mem().dynamic(base + [END], final=True).done()
    fl, fd = fitted_lengths(base + [END])

    def bad_dyn(tokens=None, lit=fl, dist=fd, data=text, **kw):
        w = Deflate().dynamic(base + [END] if tokens is None else tokens, lit, dist, True, **kw)
        return bc_member(w.getvalue(), data)
    c.append(pair("btype_3", bc_member(Deflate().fixed(base + [END], True, btype=3).getvalue(), text), good))
    gs = Mem().stored(text, True).done()
    c.append(pair("stored_len_nlen", bc_member(Deflate().stored(text, True, nlen=len(text)).getvalue(), text), gs))
    c.append(pair("stored_len_beyond_isize", bc_member(gs.body, text[:-1]), gs))
    for n in (287, 288):
        c.append(pair(f"hlit_{n}", bad_dyn(lit=fl + [0] * (n - len(fl))), gdyn))
    for n in (31, 32):
        c.append(pair(f"hdist_{n}", bad_dyn(dist=fd + [0] * (n - len(fd))), gdyn))
    # the code-length sequence of the intact block, rewritten
    seq = fl + fd
    cl_all = [4] * 13 + [5] * 6                                   # every symbol coded: 13/16 + 6/32 = 1
    assert kraft_left(cl_all) == 0
    twin = Mem().dynamic(base + [END], fl, fd, True, cl_lens=cl_all).done()
    c.append(pair("first_symbol_16", bad_dyn(header_syms=[(16, 3)] + seq[3:], cl_lens=cl_all), twin))
    c.append(pair("repeat_past_total", bad_dyn(header_syms=seq[:-2] + [(18, 11)], cl_lens=cl_all), twin))
    no_eob = list(fl)
    no_eob[256], no_eob[250] = 0, fl[256]
    c.append(pair("no_eob_code", bad_dyn(tokens=base + [250], lit=no_eob), gdyn))
    # HCLEN 4 sends lengths for 16, 17, 18 and 0 only: every length is 0, EOB included
    c.append(pair("no_eob_code_hclen_4",
                  bad_dyn(tokens=[], lit=[0] * 257, dist=[0], header_syms=[(18, 138), (18, 120)],
                          cl_lens=[1 if s in (0, 18) else 0 for s in range(19)], hclen=4), gdyn))
    over_cl = list(cl_all)
    over_cl[0] = 3
    c.append(pair("oversubscribed_cl", bad_dyn(cl_lens=over_cl), twin))
    over = list(fl)
    over[[s for s in range(256) if fl[s] == max(fl)][0]] -= 1
    c.append(pair("oversubscribed_literals", bad_dyn(lit=over), gdyn))
    c.append(pair("oversubscribed_distances", bad_dyn(dist=[1, 1, 1] + fd[3:]), gdyn))
    for s in (286, 287):
        c.append(pair(f"fixed_symbol_{s}", bc_member(Deflate().fixed(base + [fixed_raw(s), END], True).getvalue(), text), good))
    for d in (30, 31):
        w = Deflate().fixed(base + [fixed_raw(257), Raw(rev(d, 5), 5), END], True)
        c.append(pair(f"fixed_distance_{d}", bc_member(w.getvalue(), text + text[-3:]), good))
    w = Deflate().fixed(lits(b"abcde") + [fixed_raw(257), Raw(rev(4, 5), 5), Raw(1, 1), END], True)  # code 4: 5 + extra 1 = 6
    c.append(pair("distance_p_plus_1", bc_member(w.getvalue(), b"abcdeabc"), good))
    more = Mem().fixed(base + [120, END], True).done()
    c.append(pair("literal_past_isize", bc_member(more.body, text), good, match=SIZE))
    more = Mem().fixed(base + [(3, 1), END], True).done()
    c.append(pair("copy_past_isize", bc_member(more.body, more.data[:-1]), good, match=SIZE))
    c.append(pair("eob_short_of_isize", bc_member(good.body, text + b"!"), good, match=SIZE))
    c.append(pair("no_bfinal", bc_member(Deflate().fixed(base + [END], False).getvalue(), text), good))
    c.append(pair("spare_byte_before_trailer", bc_member(good.body, text, spare=b"\0"), good))
    c.append(pair("crc_flipped", bc_member(good.body, text, crc=0x5A5A5A5A), good, match="CRC"))
    # ---- incomplete code sets (zlib refuses them; a lone 1-bit code is the exception, see the valid table)
    a_eob = [0] * 257
    a_eob[97], a_eob[256] = 2, 1                                  # EOB 0, a 10; 11 is no code
    gl = [0] * 257
    gl[97] = gl[256] = 1
    gtwin = Mem().dynamic([97, 97, END], gl, [0], True).done()
    c.append(pair("incomplete_literals_unused", bad_dyn(tokens=[97, 97, END], lit=a_eob, dist=[0], data=b"aa"), gtwin, new=True))
    c.append(pair("incomplete_literals_used", bad_dyn(tokens=[97, Raw(3, 2), 97, END], lit=a_eob, dist=[0], data=b"aa"),
                  gtwin, new=True))
    dtoks = lits(b"ab") + [(4, 2), (3, 1), END]
    dl, _ = fitted_lengths(dtoks)
    dtwin = Mem().dynamic(dtoks, dl, [1, 1], True).done()
    c.append(pair("incomplete_distances_unused", bad_dyn(tokens=dtoks, lit=dl, dist=[2, 2], data=dtwin.data), dtwin, new=True))
    lc = canonical(dl + [0] * 31)
    used = lits(b"ab") + [(4, 2), Raw(rev(lc[257], dl[257]), dl[257]), Raw(1, 2), END]   # length 3, then the bits 1 0: no distance code
    c.append(pair("incomplete_distances_used", bad_dyn(tokens=used, lit=dl, dist=[2, 2], data=dtwin.data), dtwin, new=True))
    hole = [0] * 19
    hole[0], hole[8] = 1, 2                                       # 0: 0, 8: 10; 11 is no code
    all8 = lits(range(1, 40)) + [END]
    ctwin = Mem().dynamic(all8, LIT_ALL8, [0], True, cl_lens=CL_0_8).done()
    c.append(pair("incomplete_cl_unused", bad_dyn(tokens=all8, lit=LIT_ALL8, dist=[0], cl_lens=hole, data=ctwin.data),
                  ctwin, new=True))
    c.append(pair("incomplete_cl_used",
                  bad_dyn(tokens=all8, lit=LIT_ALL8, dist=[0], cl_lens=hole, data=ctwin.data,
                          header_syms=[0, 8, Raw(3, 2)] + [8] * 255 + [0]), ctwin, new=True))
    assert len({v.name for v in c}) == len(c)
    return c


# ---- TLZ members -------------------------------------------------------------------
Tlz = namedtuple("Tlz", "name members accepted")   # members: TlzMember list; accepted: the TLZ decoder's verdict
SEG = 2048


def seg_fill(total, rng, before, ids=6, end_with_copy=True):
    """Ops of one segment of `total` values: a few literals, then copies of 3..64
    values at distances up to min(8192, position) and stray literals between."""
    ops, done = [], 0
    while done < total:
        left = total - done
        pos = before + done
        if pos < 4 or left < 3 or (rng.random() < 0.3 and not (end_with_copy and left <= 64)):
            ops.append(("lit", int(rng.integers(0, ids))))
            done += 1
            continue
        n = left if left <= 64 else int(min(rng.integers(3, 65), left - 3))
        ops.append(("copy", n, int(rng.integers(1, min(8192, pos) + 1))))
        done += n
    return ops


def member_of(nvalues, seed, **kw):
    rng = np.random.default_rng(seed)
    segs = [seg_fill(min(SEG, nvalues - s), rng, s) for s in range(0, nvalues, SEG)]
    return tlz_member(segs, **kw)


def chain_segment(total):
    """One literal, then 64-value copies at distance 1 to the segment's end."""
    ops, left = [("lit", 3)], total - 1
    while left:
        n = min(64, left)
        if 0 < left - n < 3:
            n -= 3 - (left - n)
        ops.append(("copy", n, 1))
        left -= n
    return ops


# literal bytes of ranks 0, 1, 2 (00, 3f, 80, 40), EOB and seven length codes at
# 1..10, 11, 11 bits; eleven distance codes at 1..9, 10, 10 bits.  One step
# longer (a thirteenth / twelfth symbol) is one bit too many for the TLZ tables.
def _ladder(syms, n, top):
    out = [0] * n
    for k, s in enumerate(syms):
        out[s] = min(k + 1, top)
    assert kraft_left(out) == 0 and len(syms) == top + 1
    return out


_LEN_VALUES = [3, 4, 5, 6, 7, 8, 9, 11]                       # length codes 265, 267, 269..273, 274
_DIST_VALUES = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49]      # distance codes 3, 5, 6, ..., 15


def ladder_member(litmax, distmax):
    nl, nd = litmax - 4, distmax + 1
    lsy = [257 + len_sym(4 * v)[0] for v in _LEN_VALUES[:nl]]
    dsy = [dist_sym(4 * v)[0] for v in _DIST_VALUES[:nd]]
    assert len(set(lsy)) == nl and len(set(dsy)) == nd
    lit = _ladder([0x00, 0x3F, 0x80, 0x40, 256] + lsy, 286, litmax)
    dist = _ladder(dsy, 30, distmax)
    ops = [("lit", k % 3) for k in range(60)]
    for k in range(max(nl, nd)):
        ops.append(("copy", _LEN_VALUES[k % nl], _DIST_VALUES[k % nd]))
    nlit = max(i + 1 for i in range(286) if lit[i])
    return tlz_member([ops], lit[:nlit], dist[:max(i + 1 for i in range(30) if dist[i])])


# Multi-segment members whose output starts 4, 8 or 12 bytes past a multiple of
# 16: every segment then has many ops and full 8-value groups at a misaligned
# address, which is what the scalar paths of k_tlz_ops' emit (four records per
# store) and of k_tlz_resolve's value store need to be run at all.  (In
# members_3_1_2051 only the one-value member is misaligned: one op, one value.)
MISALIGNED = {
    "misaligned_12_members_3_2051_1": lambda: [member_of(3, 11), member_of(2051, 12), member_of(1, 13)],
    "misaligned_4_members_1_4100_5": lambda: [member_of(1, 14), member_of(4100, 15), member_of(5, 16)],
    "misaligned_8_members_2_2051_2051": lambda: [member_of(2, 17), member_of(2051, 18), member_of(2051, 19)],
}


@lru_cache(maxsize=None)
def tlz_cases():
    c = []
    rng = np.random.default_rng(77)

    def acc(name, *members):
        c.append(Tlz(name, list(members), True))

    def ref(name, *members):
        c.append(Tlz(name, list(members), False))
    acc("one_literal_id0", tlz_member([[("lit", 0)]]))
    acc("one_literal_id31", tlz_member([[("lit", 31)]]))
    for n in (2047, 2048, 2049):
        acc(f"values_{n}", member_of(n, n))
    acc("copy_lengths_3_and_64", tlz_member([[("lit", 1), ("lit", 2), ("lit", 4), ("copy", 3, 3), ("copy", 64, 2),
                                              ("copy", 3, 1), ("copy", 64, 70)]]))
    acc("distance_1_chain", tlz_member([chain_segment(SEG)]))
    acc("distance_1_chain_5_segments", tlz_member([chain_segment(SEG) for _ in range(5)]))
    four = [seg_fill(SEG, rng, s * SEG, ids=32) for s in range(4)]
    acc("distance_8192_at_8192", tlz_member(four + [[("copy", 64, 8192)] * 32]))
    acc("distance_8192_later", tlz_member(four + [[("lit", 9), ("lit", 8), ("lit", 7)] + [("copy", 64, 8192)] * 10]))
    back = [op for k in range(8) for op in (("copy", 64, 2048), ("copy", 64, 4096), ("copy", 64, 8192), ("lit", k))]
    acc("sources_1_2_4_segments_back", tlz_member(four + [back]))
    acc("seven_segments_ring_wraps", seven_segments())
    acc("copy_ends_on_segment_end", tlz_member([[("lit", 5)] * 1984 + [("copy", 64, 100)], [("copy", 3, 64), ("lit", 1)]]))
    for n in (16, 17, 23):
        acc(f"values_{n}_partial_group", member_of(n, n))
    acc("code_lengths_11_and_10", ladder_member(11, 10))
    acc("members_3_1_2051", member_of(3, 1), member_of(1, 2), member_of(2051, 3))
    for name, ms in MISALIGNED.items():
        acc(name, *ms())
    # ---- valid deflate that is not TLZ
    ref("copy_crosses_segment_end", tlz_member([[("lit", 5)] * 2046 + [("copy", 3, 7)], [("lit", 2)] * 10]))
    ref("copy_of_2_values", tlz_member([[("lit", 1), ("lit", 2), (8, 8), ("lit", 3)]]))
    ref("length_not_whole_values", tlz_member([[("lit", 1)] * 4 + [(13, 4), (15, 4)]]))
    ref("distance_not_whole_values", tlz_member([[("lit", 1), ("lit", 2), (12, 5)]]))
    for v in (32.0, 0.5, -0.0):
        ref(f"literal_{v}", tlz_member([[("lit", 1), ("lit", v), ("lit", 2)]]))
    ref("literal_code_length_12", ladder_member(12, 10))
    ref("distance_code_length_11", ladder_member(11, 11))
    two = [seg_fill(SEG, rng, 0), seg_fill(100, rng, SEG)]
    ref("block_split_in_two", tlz_member(two, split_at=1))
    ref("fixed_block", tlz_member(two, block="fixed"))
    assert len({v.name for v in c}) == len(c)
    return c


@lru_cache(maxsize=None)
def seven_segments():
    """14336 values: the resolve's value ring (10240 values) wraps in segment
    5; segments 5 and 6 copy at distance 8192."""
    rng = np.random.default_rng(78)
    segs = [seg_fill(SEG, rng, s * SEG, ids=32) for s in range(5)]
    for s in (5, 6):
        ops = []
        for k in range(31):
            ops += [("copy", 61, 8192), ("lit", (k + s) % 32), ("copy", 3, 8192 - (k % 5))]
        segs.append(ops + [("copy", SEG - 31 * 65, 8192)])
    m = tlz_member(segs)
    assert len(m.data) == 4 * 7 * SEG
    return m
