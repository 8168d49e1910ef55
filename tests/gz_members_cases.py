"""Streams for the host-side member parser (openfl_amd/csrc/gz_members.h), all
built with the writers the inflate tests already have (tests/bgzf.py,
tests/deflate_writer.py, tests/deflate_cases.py): valid member-indexed streams,
header-level refusals (one header field off per stream), every prefix of two
two-member streams, and streams that make the piecewise parse fall back.
Shared by tests/test_gz_members_cpu.py and by the recorder of
tests/golden/gz_index_parent.json:

    python -m tests.gz_members_cases OUT.json

writes, for the library it loads, what ofl_gzip_member_index says of every
stream and the workspace sizes of the sweep below."""
import ctypes
import json
import struct
import sys
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

from tests import deflate_cases as dc
from tests.bgzf import member_indexed, oz_members
from tests.deflate_writer import bc_member, tlz_member

# data: the bytes the writer put in (None where the stream is not meant to decode)
Stream = namedtuple("Stream", "name z data")

BATCH = 512 * 131072
WS_N = (1, 2, 3, 2047, 2048, 2049, 131071, 131072, 131073, BATCH - 1, BATCH, BATCH + 1, 1 << 31)
WS_MISALIGN = (0, 4, 8, 255)
INFLATE_NMEMBERS = (0, 1, 2, 511, 512, 513, 16384)

SIG = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0]) + b"BC" + struct.pack("<HH", 2, 99)


def _patch16(z, off, value):
    return z[:off] + struct.pack("<H", value) + z[off + 2:]


def _oz_not_last(m):
    """m's member with a second subfield behind the 'OZ' one."""
    z = m.z
    xlen, = struct.unpack_from("<H", z, 10)
    size, = struct.unpack_from("<I", z, 20)
    extra = b"XX" + struct.pack("<H", 2) + b"ab"
    z = z[:20] + struct.pack("<I", size + len(extra)) + z[24:]
    return _patch16(z, 10, xlen + len(extra))[:12 + xlen] + extra + z[12 + xlen:]


def _planted(n, every):
    raw = bytearray(dc.noise(n, 11))
    for off in range(100, n - 64, every):
        raw[off:off + len(SIG)] = SIG
    return bytes(raw)


@lru_cache(maxsize=None)
def streams():
    s = []

    def add(name, z, data=None):
        s.append(Stream(name, bytes(z), data))
    # ---- valid streams
    d = dc.noise(40000, 1)
    add("bgzf_short_last_member", member_indexed(d), d)              # 16384, 16384, 7232
    d = dc.noise(5000, 2)
    add("bgzf_empty_members", member_indexed(d, chunk=2000, empty_members=True), d)
    add("bgzf_empty_data", member_indexed(b""), b"")
    d = np.random.default_rng(3).integers(0, 6, 5000).astype(np.float32).tobytes()
    add("oz_members", oz_members(d, values_per_member=2049), d)     # 2049, 2049, 902 values
    for c in dc.valid_cases():
        add("valid_" + c.name, c.stream, c.data)
    for c in dc.tlz_cases():
        add("tlz_" + c.name, b"".join(m.z for m in c.members), b"".join(m.data for m in c.members))
    # ---- 'BC' and wide ('OZ' version 0) size fields
    d = dc.noise(300, 4)
    body = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = body.compress(d) + body.flush()
    for wide in (False, True):
        w = "wide" if wide else "bc"
        z = bc_member(body, d, wide=wide)
        add(f"{w}_size_right", z, d)
        add(f"{w}_size_too_small", bc_member(body, d, wide=wide, size_field=27))
        add(f"{w}_size_too_large", bc_member(body, d, wide=wide, size_field=len(z) + 10))
        add(f"{w}_size_stream_length", bc_member(body, d, wide=wide, size_field=len(z)), d if wide else None)
    # ---- TLZ headers with one field off: members, but not TLZ ones (or no members at all)
    def m(**kw):
        return dc.member_of(2049, 5, **kw)
    good = m()
    ln, = struct.unpack_from("<H", good.z, 14)
    add("oz_good", good.z, good.data)
    add("oz_sublen_past_xlen", _patch16(good.z, 14, ln + 1))
    add("oz_xlen_past_stream", _patch16(good.z, 10, 0xFFFF))
    add("oz_version_0", m(version=0).z, good.data)
    add("oz_seglog_10", m(seglog=10).z, good.data)
    add("oz_nseg_0", m(segbits=[]).z, good.data)
    add("oz_nseg_65", m(segbits=list(range(65))).z, good.data)
    add("oz_nseg_field_3", m(nseg=3).z, good.data)
    add("oz_nseg_3_for_2049_values", m(segbits=good.segbits + [good.segbits[-1] + 1]).z, good.data)
    add("oz_values_not_isize", m(nval=2048).z, good.data)
    add("oz_isize_not_whole_values", m(isize=len(good.data) + 1).z)
    add("oz_not_last_subfield", _oz_not_last(good), good.data)
    # ---- every prefix of two two-member streams
    two = dc.small(1).z + dc.small(2).z
    for k in range(len(two) + 1):
        add(f"prefix_bc_{k}", two[:k])
    two = dc.member_of(3, 1).z + dc.member_of(1, 2).z
    for k in range(len(two) + 1):
        add(f"prefix_oz_{k}", two[:k])
    # ---- for the piecewise parse at 4 threads, 256-byte pieces
    d = dc.noise(8000, 6)
    add("pieces_all_link", member_indexed(d, chunk=500, level=0), d)
    d = _planted(6000, 700)
    add("pieces_fake_signatures", member_indexed(d, chunk=1500, level=0), d)
    d = dc.noise(2000, 7)
    add("pieces_without_header", member_indexed(d, chunk=60000, level=0), d)
    assert len({x.name for x in s}) == len(s)
    return s


def library_index(z):
    """ofl_gzip_member_index of the loaded library -> the record the golden file holds."""
    from openfl_amd import _lib
    L = _lib.lib()
    src = np.frombuffer(z, np.uint8) if z else np.zeros(1, np.uint8)
    cap = len(z) // 26 + 1
    idx = np.zeros((cap, 4), np.int64)
    nm, tot, mx, tl = ctypes.c_int64(), ctypes.c_size_t(), ctypes.c_uint32(), ctypes.c_int()
    rc = L.ofl_gzip_member_index(src.ctypes.data, len(z), idx.ctypes.data, cap, ctypes.byref(nm), ctypes.byref(tot),
                                 ctypes.byref(mx), ctypes.byref(tl))
    if rc:
        return {"rc": rc, "n": 0, "total": 0, "all_tlz": 0, "index": []}
    return {"rc": 0, "n": nm.value, "total": tot.value, "all_tlz": tl.value,
            "index": [int(v) for v in idx[:nm.value].ravel()]}


def library_sizes():
    from openfl_amd import _lib
    L = _lib.lib()
    return {"ranks": {str(n): [int(L.ofl_gzip_ranks_workspace_bytes(n)), int(L.ofl_gzip_ranks_bound(n))] for n in WS_N},
            "inflate": {str(n): int(L.ofl_inflate_tlz_workspace_bytes(n)) for n in INFLATE_NMEMBERS}}


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump({"streams": {x.name: library_index(x.z) for x in streams()}, "sizes": library_sizes()}, f,
                  separators=(",", ":"))
        f.write("\n")
