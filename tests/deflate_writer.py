"""Designed deflate streams for the inflate tests (RFC 1951 / RFC 1952), in
plain Python: a bit writer, canonical codes from explicit code lengths, the
three block types from explicit token lists, the member headers the inflate
kernels index ('BC' and the TLZ 'OZ' subfield of csrc/gz_format.h), a
ten-line LZ77 interpreter that gives the expected bytes without zlib, and a
small reader of dynamic blocks that lists what an encoder wrote.  Test data
only: no device code.

Tokens: an int 0..255 is a literal; (length, distance) is a copy in bytes;
END is the end-of-block symbol; Raw(bits, n) puts n bits verbatim (LSB first);
SymCopy(lsym, lextra, dsym, dextra) is a copy by explicit length / distance
symbols and extra-bit values (length 258 as code 284 + 31, for instance)."""
import heapq
import struct
import zlib
from collections import namedtuple

END = "end"
Raw = namedtuple("Raw", "bits n")
SymCopy = namedtuple("SymCopy", "lsym lextra dsym dextra")

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CLORD = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def len_sym(length):
    """(symbol - 257, extra value) of a copy length; 258 is code 285."""
    if length == 258:
        return 28, 0
    s = max(i for i in range(28) if LBASE[i] <= length)
    assert length - LBASE[s] < (1 << LEXT[s])
    return s, length - LBASE[s]


def dist_sym(dist):
    s = max(i for i in range(30) if DBASE[i] <= dist)
    assert dist - DBASE[s] < (1 << DEXT[s])
    return s, dist - DBASE[s]


def as_symcopy(tok):
    if isinstance(tok, SymCopy):
        return tok
    ls, lx = len_sym(tok[0])
    ds, dx = dist_sym(tok[1])
    return SymCopy(257 + ls, lx, ds, dx)


def canonical(lens):
    """Canonical Huffman codes (RFC 1951 3.2.2) of explicit code lengths, as
    integers to be sent most significant bit first.  Defined for any lengths:
    an over-subscribed or incomplete set gets the same arithmetic."""
    cnt = [0] * 17
    for ln in lens:
        cnt[ln] += 1
    cnt[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    out = []
    for ln in lens:
        out.append(nxt[ln] if ln else 0)
        nxt[ln] += 1 if ln else 0
    return out


def kraft_left(lens):
    """Unused code space in units of 2^-15: 0 complete, < 0 over-subscribed."""
    return (1 << 15) - sum(1 << (15 - ln) for ln in lens if ln)


def complete_by_zlib(lens, is_cl=False):
    """zlib's inflate_table verdict on a code set: complete, or empty, or (not
    for the code-length alphabet) incomplete with a longest code of 1 bit."""
    left, mx = kraft_left(lens), max(list(lens) + [0])
    return left == 0 or mx == 0 or (left > 0 and mx == 1 and not is_cl)


def limited_lengths(freq, maxlen):
    """Code lengths <= maxlen for the symbols with freq > 0: Huffman by a heap,
    then the Kraft sum repaired.  A lone symbol gets a partner (symbol 0 or 1)
    so that the set is complete; Kraft equality is asserted."""
    used = [s for s, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    if not used:
        return lens
    if len(used) == 1:
        assert len(freq) >= 2
        lens[used[0]] = 1
        lens[1 if used[0] == 0 else 0] = 1
        return lens
    heap = [(freq[s], s, (s,)) for s in used]
    heapq.heapify(heap)
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        for s in a[2] + b[2]:
            lens[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    for s in used:
        lens[s] = min(lens[s], maxlen)
    full = 1 << maxlen
    k = sum(1 << (maxlen - lens[s]) for s in used)
    while k > full:                                                # lengthen the longest, rarest code below maxlen
        s = next(s for s in sorted(used, key=lambda s: (-lens[s], freq[s], s)) if lens[s] < maxlen)
        k -= 1 << (maxlen - lens[s] - 1)
        lens[s] += 1
    while k < full:                                                # shorten where it still fits
        s = next(s for s in sorted(used, key=lambda s: (-lens[s], -freq[s], s))
                 if lens[s] > 1 and k + (1 << (maxlen - lens[s])) <= full)
        k += 1 << (maxlen - lens[s])
        lens[s] -= 1
    assert k == full and kraft_left(lens) == 0 and max(lens) <= maxlen
    return lens


class BitWriter:
    """Bits LSB first into bytes; Huffman codes MSB first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def bits(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        rev = 0
        for _ in range(n):
            rev = (rev << 1) | (code & 1)
            code >>= 1
        self.bits(rev, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw_bytes(self, b):
        assert self.n == 0
        self.out += b

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


class Deflate(BitWriter):
    """Blocks appended to one bit stream."""

    def stored(self, data, final, nlen=None):
        self.bits(1 if final else 0, 1)
        self.bits(0, 2)
        self.align()
        self.bits(len(data), 16)
        self.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self.raw_bytes(data)
        return self

    def symbols(self, tokens, lit_lens, dist_lens, mark=None):
        lc, dc = canonical(lit_lens), canonical(dist_lens)
        for k, t in enumerate(tokens):
            if mark is not None:
                mark(k, self.bitpos)
            if isinstance(t, Raw):
                self.bits(t.bits, t.n)
            elif t == END:
                assert lit_lens[256]
                self.code(lc[256], lit_lens[256])
            elif isinstance(t, int):
                assert lit_lens[t], f"literal {t} has no code"
                self.code(lc[t], lit_lens[t])
            else:
                c = as_symcopy(t)
                assert lit_lens[c.lsym] and dist_lens[c.dsym], f"copy {t} has no code"
                self.code(lc[c.lsym], lit_lens[c.lsym])
                self.bits(c.lextra, LEXT[c.lsym - 257])
                self.code(dc[c.dsym], dist_lens[c.dsym])
                self.bits(c.dextra, DEXT[c.dsym])

    def fixed(self, tokens, final, btype=1, mark=None):
        self.bits(1 if final else 0, 1)
        self.bits(btype, 2)
        self.symbols(tokens, FIXED_LIT, FIXED_DIST, mark)
        return self

    def dynamic(self, tokens, lit_lens, dist_lens, final, cl_lens=None, header_syms=None, hclen=None, mark=None):
        """lit_lens / dist_lens: HLIT and HDIST follow from their lengths (257..288
        and 1..32 fit the 5-bit fields, so the invalid counts can be written).
        header_syms: the code-length sequence as ints 0..15 and (16 | 17 | 18,
        count) pairs; default: every length plainly.  cl_lens: the 19 lengths of
        the code-length alphabet by symbol; default: a complete code for the
        symbols used.  hclen: the number of code-length lengths sent."""
        assert 257 <= len(lit_lens) <= 288 and 1 <= len(dist_lens) <= 32
        if header_syms is None:
            header_syms = list(lit_lens) + list(dist_lens)
        syms = [h if isinstance(h, int) else h[0] for h in header_syms]
        if cl_lens is None:
            freq = [0] * 19
            for s in syms:
                freq[s] += 1
            cl_lens = limited_lengths(freq, 7)
        assert len(cl_lens) == 19 and max(cl_lens) <= 7
        if hclen is None:
            hclen = max([4] + [i + 1 for i in range(19) if cl_lens[CLORD[i]]])
        self.bits(1 if final else 0, 1)
        self.bits(2, 2)
        self.bits(len(lit_lens) - 257, 5)
        self.bits(len(dist_lens) - 1, 5)
        self.bits(hclen - 4, 4)
        for i in range(hclen):
            self.bits(cl_lens[CLORD[i]], 3)
        cc = canonical(cl_lens)
        for h in header_syms:
            s = h if isinstance(h, int) else h[0]
            if isinstance(h, Raw):
                self.bits(h.bits, h.n)
                continue
            assert cl_lens[s], f"code-length symbol {s} has no code"
            self.code(cc[s], cl_lens[s])
            if s == 16:
                self.bits(h[1] - 3, 2)
            elif s == 17:
                self.bits(h[1] - 3, 3)
            elif s == 18:
                self.bits(h[1] - 11, 7)
        self.symbols(tokens, list(lit_lens) + [0] * (288 - len(lit_lens)), list(dist_lens) + [0] * (32 - len(dist_lens)),
                     mark)
        return self


def expand(tokens):
    """The bytes a token list stands for: a plain LZ77 interpreter."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif t != END and not isinstance(t, Raw):
            c = as_symcopy(t)
            n, d = LBASE[c.lsym - 257] + c.lextra, DBASE[c.dsym] + c.dextra
            assert 1 <= d <= len(out)
            for _ in range(n):
                out.append(out[-d])
    return bytes(out)


def token_freqs(tokens):
    lit, dist = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, Raw):
            continue
        if t == END:
            lit[256] += 1
        elif isinstance(t, int):
            lit[t] += 1
        else:
            c = as_symcopy(t)
            lit[c.lsym] += 1
            dist[c.dsym] += 1
    return lit, dist


def fitted_lengths(tokens, litmax=15, distmax=15):
    """Complete code sets (limited_lengths) for an arbitrary token list,
    trimmed to the shortest HLIT / HDIST."""
    lf, df = token_freqs(tokens)
    lf[256] = max(lf[256], 1)
    ll, dl = limited_lengths(lf, litmax), limited_lengths(df, distmax)
    nl = max(257, max(i + 1 for i in range(286) if ll[i]))
    nd = max([1] + [i + 1 for i in range(30) if dl[i]])
    return ll[:nl], dl[:nd]


def bc_member(deflate_bytes, data, crc=None, isize=None, size_field=None, wide=False, spare=b""):
    """A member with tests/bgzf.py's 'BC' header (member size - 1 in 16 bits)
    around given deflate data, then CRC-32 and ISIZE of `data`.  wide: members
    above 64 KiB carry their size in 32 bits instead, in an 'OZ' subfield of
    version 0 (the index reads its size; no decoder takes it for TLZ).
    spare: bytes between the deflate data and the trailer."""
    crc = zlib.crc32(data) if crc is None else crc
    isize = len(data) if isize is None else isize
    tail = deflate_bytes + spare + struct.pack("<II", crc & 0xFFFFFFFF, isize)
    if wide:
        size = 28 + len(tail)
        return bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 16, 0]) + b"OZ" + struct.pack(
            "<HBBHII", 12, 0, 11, 0, size if size_field is None else size_field, 0) + tail
    size = 18 + len(tail)
    assert size <= 65536
    return bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0]) + b"BC" + struct.pack(
        "<HH", 2, size - 1 if size_field is None else size_field) + tail


def rank_bytes(rank):
    return struct.pack("<f", float(rank))


TlzMember = namedtuple("TlzMember", "z data tokens segbits body")


def tlz_tokens(segments):
    """Byte-level tokens of per-segment op lists: ('lit', id) is the 4 bytes of
    float32(id), ('copy', n_values, dist_values) a copy of whole values; any
    other entry is a byte-level token passed through.  -> (tokens, index of
    every segment's first token)."""
    tokens, first = [], []
    for ops in segments:
        first.append(len(tokens))
        for op in ops:
            if isinstance(op, tuple) and op and op[0] == "lit":
                tokens += list(rank_bytes(op[1]))
            elif isinstance(op, tuple) and op and op[0] == "copy":
                tokens.append((4 * op[1], 4 * op[2]))
            else:
                tokens.append(op)
    return tokens, first


def tlz_member(segments, lit_lens=None, dist_lens=None, block="dynamic", split_at=None, litmax=11, distmax=10,
               nseg=None, size=None, nval=None, segbits=None, version=1, seglog=11, crc=None, isize=None):
    """One TLZ member as k_tlz_encode writes it: the 28-byte header with the
    'OZ' subfield (version, log2 segment, segment count, member bytes, value
    count), the table of every segment's first-symbol bit offset, ONE final
    dynamic block, CRC-32 and ISIZE.  block='fixed' and split_at (a segment
    index at which the block ends and a second one, with the same codes,
    begins) write valid deflate that is not TLZ; the keyword overrides replace
    header fields."""
    tokens, first = tlz_tokens(segments)
    body_tokens = tokens + [END]
    data = expand(body_tokens)
    if lit_lens is None or dist_lens is None:
        fl, fd = fitted_lengths(body_tokens, litmax, distmax)
        lit_lens = fl if lit_lens is None else lit_lens
        dist_lens = fd if dist_lens is None else dist_lens
    pos = {}
    w = Deflate()

    def mark(base):
        return lambda k, bit: pos.__setitem__(base + k, bit)
    if block == "fixed":
        w.fixed(body_tokens, True, mark=mark(0))
    elif split_at is not None:
        cut = first[split_at]
        w.dynamic(tokens[:cut] + [END], lit_lens, dist_lens, False, mark=mark(0))
        pos.pop(cut, None)
        w.dynamic(body_tokens[cut:], lit_lens, dist_lens, True, mark=mark(cut))
    else:
        w.dynamic(body_tokens, lit_lens, dist_lens, True, mark=mark(0))
    body = w.getvalue()
    table = [pos[f] for f in first] if segbits is None else list(segbits)
    ns = len(table)
    ln = 12 + 4 * ns
    total = 28 + 4 * ns + len(body) + 8
    hdr = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF]) + struct.pack("<H", 4 + ln) + b"OZ" + struct.pack(
        "<HBBHII", ln, version, seglog, ns if nseg is None else nseg, total if size is None else size,
        len(data) // 4 if nval is None else nval)
    z = hdr + b"".join(struct.pack("<I", b) for b in table) + body + struct.pack(
        "<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize)
    return TlzMember(z, data, body_tokens, table, body)


# ---- reader ------------------------------------------------------------------
class _Bits:
    def __init__(self, data, bit=0):
        self.d = data + bytes(8)
        self.p = bit

    def peek(self, n):
        q = self.p >> 3
        return (int.from_bytes(self.d[q:q + 8], "little") >> (self.p & 7)) & ((1 << n) - 1)

    def get(self, n):
        v = self.peek(n)
        self.p += n
        return v


def _table(lens):
    """{(length, code)} -> symbol as a flat look-up over max-length reversed bits."""
    mx = max(list(lens) + [0])
    tab = [None] * (1 << mx) if mx else []
    for s, (ln, c) in enumerate(zip(lens, canonical(lens))):
        if ln:
            rev = int(format(c, f"0{ln}b")[::-1], 2)
            for k in range(rev, 1 << mx, 1 << ln):
                tab[k] = (s, ln)
    return tab, mx


def _sym(b, tab, mx):
    e = tab[b.peek(mx)] if mx else None
    if e is None:
        raise ValueError(f"no code at bit {b.p}")
    b.p += e[1]
    return e[0]


def read_member(z, off=0):
    """Read the member at z[off:]: header fields, then its dynamic blocks symbol
    by symbol.  -> dict: kind ('BC' | 'OZ'), size, version, seglog, nseg, nval,
    segbits, crc, isize, data_off, data_len, and blocks: a list of dicts
    (bfinal, cl_lens, lit_lens, dist_lens, tokens), tokens being (bit position
    from the first bit of the deflate data, token) pairs.  Raises ValueError on
    a stored, fixed or reserved block type and on bits that are no code."""
    h = z[off:]
    if h[:4] != b"\x1f\x8b\x08\x04":
        raise ValueError("not a member with an extra field")
    xlen = struct.unpack_from("<H", h, 10)[0]
    m = {"kind": None, "segbits": []}
    q = 12
    while q + 4 <= 12 + xlen:
        sid, sl = h[q:q + 2], struct.unpack_from("<H", h, q + 2)[0]
        if sid == b"BC":
            m.update(kind="BC", size=struct.unpack_from("<H", h, q + 4)[0] + 1)
        elif sid == b"OZ":
            ver, sg, ns, size, nval = struct.unpack_from("<BBHII", h, q + 4)
            m.update(kind="OZ", version=ver, seglog=sg, nseg=ns, size=size, nval=nval,
                     segbits=list(struct.unpack_from(f"<{(sl - 12) // 4}I", h, q + 16)))
        q += 4 + sl
    if m["kind"] is None:
        raise ValueError("no size subfield")
    m["data_off"] = off + 12 + xlen
    m["data_len"] = m["size"] - 12 - xlen - 8
    m["crc"], m["isize"] = struct.unpack_from("<II", h, m["size"] - 8)
    b = _Bits(bytes(h[12 + xlen:12 + xlen + m["data_len"]]))
    blocks = []
    while True:
        bfinal, btype = b.get(1), b.get(2)
        if btype != 2:
            raise ValueError(f"block type {btype}: only dynamic blocks are read")
        nlit, ndist, ncl = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
        cl = [0] * 19
        for i in range(ncl):
            cl[CLORD[i]] = b.get(3)
        tab, mx = _table(cl)
        lens = []
        while len(lens) < nlit + ndist:
            s = _sym(b, tab, mx)
            if s < 16:
                lens.append(s)
            elif s == 16:
                if not lens:
                    raise ValueError("repeat with nothing before it")
                lens += [lens[-1]] * (3 + b.get(2))
            elif s == 17:
                lens += [0] * (3 + b.get(3))
            else:
                lens += [0] * (11 + b.get(7))
        if len(lens) != nlit + ndist:
            raise ValueError("a repeat runs past the code lengths")
        ll, dl = lens[:nlit], lens[nlit:]
        lt, lmx = _table(ll)
        dt, dmx = _table(dl)
        toks = []
        while True:
            at = b.p
            s = _sym(b, lt, lmx)
            if s < 256:
                toks.append((at, s))
            elif s == 256:
                toks.append((at, END))
                break
            else:
                if s > 285:
                    raise ValueError("length symbol 286 / 287")
                lx = b.get(LEXT[s - 257])
                ds = _sym(b, dt, dmx)
                if ds > 29:
                    raise ValueError("distance symbol 30 / 31")
                dx = b.get(DEXT[ds])
                toks.append((at, (LBASE[s - 257] + lx, DBASE[ds] + dx)))
        blocks.append({"bfinal": bfinal, "cl_lens": cl, "lit_lens": ll, "dist_lens": dl, "tokens": toks})
        if bfinal:
            break
    m["blocks"] = blocks
    m["end_bit"] = b.p
    return m
