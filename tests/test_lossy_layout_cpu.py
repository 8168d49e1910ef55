"""The lossy kernels' host-only header (openfl_amd/csrc/lossy_layout.h) checked
without a GPU: tests/lossy_layout_check.cpp includes it as the library does and
prints, for the arenas of tests/lossy_layout_cases.py, the chunk table, every
family's workspace regions and cleared spans, and the totals.  Three things
must agree for every case: the checker, the library's *_workspace_bytes, and
the values recorded from the library of the commit before the layouts moved
into the header (tests/golden/lossy_layout_parent.json).  The table and the
regions are checked against the restatement in the cases module, not against
the header.  The golden file also holds the (return code, last error) of the
calls the parent refused before its first HIP call; the library must still
answer each the same.  The same program runs under AddressSanitizer and UBSan.

The golden file was made on the CPU from a build of the parent commit:
`OFL_CODEC_LIB=<parent's libofl_codec.so> python -m tests.lossy_layout_cases`."""
import json
import os
import shutil
import subprocess

import pytest

from tests import lossy_layout_cases as lc

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
FAMILY_REGIONS = {"kmeans": ["td", "st", "hc", "hs", "part", "seeds"], "topk": ["td", "st", "hist", "blk"],
                  "lut": ["td", "nk", "keys", "vals"], "ternary": ["td", "ranks3"]}
SLACK = 256


def _cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError("no C++ compiler (CXX, c++, g++, clang++)")


def _build(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags,
                    "-I", os.path.join(ROOT, "openfl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "lossy_layout_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe):
    run = subprocess.run([exe], input=lc.checker_input(), capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    out, cur = {}, None
    for line in run.stdout.splitlines():
        f = line.split()
        if f[0] == "case":
            cur = out[f[1]] = {"table": [], "layouts": {}, "regions": {}, "spans": {}}
        elif f[0] == "C":
            cur["err"], cur["blocks"] = int(f[1]), int(f[2])
        elif f[0] == "t":
            cur["table"].append(tuple(int(v) for v in f[1:]))
        elif f[0] == "L":
            cur["layouts"][f[1]] = (int(f[2]), int(f[3]))
        elif f[0] == "r":
            cur["regions"].setdefault(f[1], []).append((f[2], int(f[3]), int(f[4])))
        elif f[0] == "z":
            cur["spans"][f[1]] = (int(f[3]), int(f[4]), f[5], f[6])
        elif f[0] == "S":
            cur["single"] = int(f[1])
    return out


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return _run(_build(tmp_path_factory.mktemp("lossy_layout"), "lossy_layout_check"))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "lossy_layout_parent.json")) as f:
        return json.load(f)


def test_cases_are_the_designed_and_golden_ones(golden):
    cs = lc.cases()
    assert sorted(c.name for c in cs) == sorted(golden["sizes"]) and len(cs) == 2 * len(lc.TS) * len(lc.GAPS)
    assert {len(c.numels) for c in cs} == set(lc.TS) and {c.max_nk for c in cs} == set(lc.MAX_NK)
    assert {n for c in cs for n in c.numels} == set(lc.NUMELS_ZERO)
    gaps = {o1 - o0 - n0 for c in cs for o0, n0, o1 in zip(c.offsets, c.numels, c.offsets[1:])}
    assert gaps == set(lc.GAPS)


def test_checker_library_and_parent_agree(dump, golden):
    for c in lc.cases():
        got, want = dump[c.name], golden["sizes"][c.name]
        mine = {"kmeans": got["layouts"]["kmeans"][1], "topk": got["layouts"]["topk"][1],
                "ternary": got["layouts"]["ternary"][1], "single": got["single"]}
        lib = lc.library_sizes(c)
        for key, val in mine.items():
            assert val == lib[key] == want[key], (c.name, key)
        assert got["layouts"]["lut"][1] == lib["lut"][str(c.max_nk)], c.name
        assert lib["lut"] == want["lut"], c.name
        for fam, (end, total) in got["layouts"].items():
            assert total == end + SLACK, (c.name, fam)


def test_chunk_table_is_the_running_sum(dump):
    for c in lc.cases():
        got = dump[c.name]
        blk0, nblk, blocks = lc.chunk_table(c.numels)
        assert got["err"] == 0 and got["blocks"] == blocks, c.name
        assert got["table"] == list(zip(c.offsets, c.numels, blk0, nblk)), c.name


def test_regions_are_aligned_ascending_and_disjoint(dump):
    for c in lc.cases():
        for fam, regions in dump[c.name]["regions"].items():
            assert [r[0] for r in regions] == FAMILY_REGIONS[fam], (c.name, fam)
            at = 0
            for name, off, size in regions:
                assert off % 256 == 0 and size % 256 == 0 and size > 0, (c.name, fam, name)
                assert off == at, (c.name, fam, name)        # ascending, disjoint, no hole
                at = off + size
            assert at == dump[c.name]["layouts"][fam][0], (c.name, fam)


def test_cleared_spans_cover_exactly_their_regions(dump):
    for c in lc.cases():
        got = dump[c.name]
        assert set(got["spans"]) == {"kmeans", "topk"}
        for fam, (off, size, first, last) in got["spans"].items():
            reg = {name: (o, s) for name, o, s in got["regions"][fam]}
            assert off == reg[first][0] and off + size == sum(reg[last]), (c.name, fam)
        assert (got["spans"]["kmeans"][2:], got["spans"]["topk"][2:]) == (("st", "hs"), ("hist", "hist"))
        names = FAMILY_REGIONS["kmeans"]
        assert names[names.index("st"):names.index("hs") + 1] == ["st", "hc", "hs"]   # states + both histograms


def test_refusals_equal_the_parents(golden):
    got = lc.run_refusals()
    assert sorted(got) == sorted(golden["refusals"]) and len(got) == 28
    for name, pair in got.items():
        assert pair == golden["refusals"][name], name
        assert pair[0] in (-1, -3) and pair[1], name          # OFL_EINVAL / OFL_ESPACE, with a message


def test_lut_batch_refuses_what_the_parent_followed_or_truncated():
    """The one behaviour change: NULL offsets / numels / nk, a tensor of 2^47
    elements, and two tensors of 2^46 (each legal, 2^31 blocks together) are
    OFL_EINVAL before any HIP call."""
    got = lc.run_refusals(1)
    assert set(got) == {"lut_no_offsets", "lut_no_numels", "lut_no_nk", "lut_2p47_elements", "lut_2p31_blocks"}
    for name, (rc, msg) in got.items():
        assert rc == -1 and msg.startswith("lut:"), (name, rc, msg)
    assert "length" in got["lut_2p47_elements"][1] and "batch too large" in got["lut_2p31_blocks"][1]


def test_sanitized(tmp_path, dump):
    """The same stand-alone program under AddressSanitizer and UBSan: clean, and the same output."""
    exe = _build(tmp_path, "lossy_layout_check_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert _run(exe) == dump
