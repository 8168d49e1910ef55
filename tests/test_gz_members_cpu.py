"""The gzip codec's host-only code (openfl_amd/csrc/gz_format.h, gz_members.h)
checked without a GPU: tests/gz_members_check.cpp includes the two headers the
library includes and parses the streams of tests/gz_members_cases.py three
ways (the serial walk, the piecewise parse as the library calls it, the
piecewise parse with 256-byte pieces).  Three things must agree for every
stream: the checker, the library's ofl_gzip_member_index, and the index
recorded from the commit before the parser moved into the header
(tests/golden/gz_index_parent.json).  zlib is the independent reference for
the valid streams.  The same program runs under AddressSanitizer and UBSan on
heap copies of exactly each stream's length."""
import json
import os
import shutil
import subprocess
import zlib

import pytest

from tests import gz_members_cases as gc

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
MODES = ("serial", "library", "small")
TLZ_BIT = 1 << 62


def _cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError("no C++ compiler (CXX, c++, g++, clang++)")


def _build(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-pthread",
                    "-I", os.path.join(ROOT, "openfl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "gz_members_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe):
    text = "".join(f"{s.name} {s.z.hex() or '-'}\n" for s in gc.streams())
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    parsed = {m: {} for m in MODES}
    layouts, inflate, cur = [], {}, None
    for line in run.stdout.splitlines():
        f = line.split()
        if f[0] == "stream":
            cur = parsed[f[2]][f[1]] = {"index": []}
        elif f[0] == "R":
            cur.update(rc=int(f[1]), n=int(f[2]), total=int(f[3]), all_tlz=int(f[4]))
        elif f[0] == "M":
            cur["index"] += [int(v) for v in f[1:]]
        elif f[0] == "W":
            layouts.append({"n": int(f[1]), "misalign": int(f[2]), "regions": []})
        elif f[0] == "r":
            layouts[-1]["regions"].append((f[1], int(f[2]), int(f[3])))
        elif f[0] == "E":
            layouts[-1].update(end=int(f[1]), bound=int(f[2]))
        elif f[0] == "I":
            inflate[int(f[1])] = tuple(int(v) for v in f[2:])
    return parsed, layouts, inflate


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return _run(_build(tmp_path_factory.mktemp("gz_members"), "gz_members_check"))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "gz_index_parent.json")) as f:
        return json.load(f)


def test_streams_are_the_golden_ones(golden):
    assert [s.name for s in gc.streams()] == list(golden["streams"])


@pytest.mark.parametrize("mode", MODES)
def test_checker_equals_parent(dump, golden, mode):
    """Every stream's return code, member count, total, all_tlz and index words; the
    piecewise parses give what the serial walk gives."""
    got = dump[0][mode]
    assert list(got) == list(golden["streams"])
    for name, want in golden["streams"].items():
        assert got[name] == want, f"{mode}: {name}"


def test_library_equals_parent(golden):
    for s in gc.streams():
        assert gc.library_index(s.z) == golden["streams"][s.name], s.name


def test_golden_is_what_the_cases_mean(golden):
    """The recorded verdicts are the designed ones: which streams are refused,
    which members count as TLZ, and prefixes accepted exactly at member boundaries."""
    g = golden["streams"]
    for name in ("bc_size_too_small", "bc_size_too_large", "bc_size_stream_length", "wide_size_too_small",
                 "wide_size_too_large", "oz_sublen_past_xlen", "oz_xlen_past_stream"):
        assert g[name]["rc"] == -4, name
    assert g["oz_good"]["all_tlz"] == 1 and g["oz_members"]["all_tlz"] == 1
    for name in ("oz_version_0", "oz_seglog_10", "oz_nseg_0", "oz_nseg_65", "oz_nseg_field_3", "oz_nseg_3_for_2049_values",
                 "oz_values_not_isize", "oz_isize_not_whole_values", "oz_not_last_subfield", "wide_size_right"):
        assert (g[name]["rc"], g[name]["n"], g[name]["all_tlz"]) == (0, 1, 0), name
    for c in gc.dc.tlz_cases():
        assert g["tlz_" + c.name]["all_tlz"] == 1, c.name      # TLZ by their headers, whatever the decoder says
    for kind, ends in (("bc", [len(gc.dc.small(1).z), len(gc.dc.small(1).z) + len(gc.dc.small(2).z)]),
                       ("oz", [len(gc.dc.member_of(3, 1).z), len(gc.dc.member_of(3, 1).z) + len(gc.dc.member_of(1, 2).z)])):
        for k in range(ends[-1] + 1):
            want = (0, ([0] + ends).index(k)) if k in [0] + ends else (-4, 0)
            assert (g[f"prefix_{kind}_{k}"]["rc"], g[f"prefix_{kind}_{k}"]["n"]) == want, (kind, k)
    assert g["pieces_fake_signatures"]["n"] == 4 and g["pieces_without_header"]["n"] == 1


def test_valid_streams_against_zlib(dump):
    """Independent of the golden file: each member's deflate range inflates (raw,
    zlib) to the bytes the writer put in, with their CRC-32 and size in the record."""
    for s in gc.streams():
        if s.data is None:
            continue
        r = dump[0]["serial"][s.name]
        assert r["rc"] == 0 and r["total"] == len(s.data), s.name
        for k in range(r["n"]):
            off, ln, out, w3 = r["index"][4 * k:4 * k + 4]
            ln &= ~TLZ_BIT
            w3 &= (1 << 64) - 1                                  # the words are signed int64
            part = s.data[out:out + (w3 & 0xFFFFFFFF)]
            assert zlib.decompress(s.z[off:off + ln], -15) == part, (s.name, k)
            assert w3 >> 32 == zlib.crc32(part), (s.name, k)
        assert sum(w & 0xFFFFFFFF for w in r["index"][3::4]) == len(s.data)


def test_workspace_layout(dump, golden):
    _, layouts, inflate = dump
    assert [(w["n"], w["misalign"]) for w in layouts] == [(n, m) for n in gc.WS_N for m in gc.WS_MISALIGN]
    align = {"slots": 256, "ops": 4, "sizes": 4, "off": 8, "running": 8, "bad": 4, "stage": 256}
    for w in layouts:
        want_end, want_bound = golden["sizes"]["ranks"][str(w["n"])]
        assert (w["end"], w["bound"]) == (want_end, want_bound), w["n"]
        spans = sorted((off, off + size, name) for name, off, size in w["regions"])
        assert len(spans) == 11     # slots, sizes, off and stage twice; ops, running, bad
        for (_, e0, n0), (s1, _, n1) in zip(spans, spans[1:]):
            assert e0 <= s1, (w["n"], w["misalign"], n0, n1)
        assert spans[-1][1] <= w["end"]
        for name, off, _ in w["regions"]:
            assert (w["misalign"] + off) % align[name.rstrip("01")] == 0, (w["n"], w["misalign"], name)
    for n in gc.INFLATE_NMEMBERS:
        assert inflate[n] == (0, 256, golden["sizes"]["inflate"][str(n)])
    assert gc.library_sizes() == golden["sizes"]


def test_sanitized(tmp_path, dump):
    """The same stand-alone program under AddressSanitizer and UBSan: clean, and the same output."""
    exe = _build(tmp_path, "gz_members_check_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert _run(exe) == dump
