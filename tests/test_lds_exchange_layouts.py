"""The lane-linear LDS exchange's address math (openfl_amd/csrc/lds_exchange.h),
checked on the host: tests/lds_exchange_check.cpp includes the header the
kernels include and replays every store and load of all 512 threads for every
layout pair that goes through exchange_half_lin."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CSRC = os.path.join(ROOT, "openfl_amd", "csrc")
PAIRS = ("RowC2 L3->L4", "RowC2 L4->L5", "DecA2 C1->C2", "DecA2 C2->C3", "RowA2 A1->A2", "RowA2 A2->A3",
         "DecC2 B1->B2", "DecC2 B2->B3", "DecC2 B3->B4")
WIDTHS = (1, 4, 1, 1, 4, 1, 4, 4, 1)   # 4: the destination's registers 0, 1 lie on the source's lanes 0, 1
ROW = re.compile(r"^pair (\w+ \S+) width (\d) image ([\d,|]+) footprint (\d+) budget (\d+) wrong (\d+) conflicts (\d+) "
                 r"misaligned (\d+) range (\d+) constexpr_ok (\d)$", re.M)


def _cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError("no C++ compiler (CXX, c++, g++, clang++)")


def _build(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC,
                    os.path.join(ROOT, "tests", "lds_exchange_check.cpp"), "-o", exe], check=True)
    return exe


def _check_output(run):
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    rows = {m[0]: m for m in ROW.findall(run.stdout)}
    assert tuple(rows) == PAIRS, run.stdout
    for name, (_, width, image, footprint, budget, wrong, conflicts, misaligned, rng, cx) in rows.items():
        # inverse permutations, no bank conflict in any lane group, aligned wide reads
        assert (int(wrong), int(conflicts), int(misaligned), int(rng), int(cx)) == (0, 0, 0, 0, 1), name
        # the padded half image of the element-indexed exchange: 2^14 + 2^9 + 2^4 floats
        assert int(budget) == 16912 and 16384 <= int(footprint) <= int(budget), name
    assert {n: int(r[1]) for n, r in rows.items()} == dict(zip(PAIRS, WIDTHS))
    # a pair whose destination lanes read along the source's rows needs no padding
    assert rows["RowC2 L3->L4"][2] == rows["DecA2 C2->C3"][2] == "64,128,256,512,1024|2048,4096,8192"
    ctl = re.search(r"^control DecA2 C1->C2 image plain wrong 0 conflicts (\d+) constexpr_ok 0$", run.stdout, re.M)
    assert ctl and int(ctl.group(1)) > 0, run.stdout  # the checker sees a conflict where there is one


def test_checker_layouts_are_the_kernels():
    """The pairs the checker walks are the two-block row kernels' layout sets
    (RowC2Set, DecA2Set, RowA2Set, DecC2Set), and the exchanges the kernels
    send through exchange_half_lin are among them."""
    src = open(os.path.join(CSRC, "eden_kernels.hip")).read()
    chk = open(os.path.join(ROOT, "tests", "lds_exchange_check.cpp")).read()
    for text in ("L3{15, 5, 6, 7, 8, 9, 10}", "L4{15, 11, 12, 13, 14, 9, 10}", "L5{15, 0, 1, 2, 3, 4, 10}",
                 "C1 = RS::L5", "L5{15, 0, 1, 2, 3, 4, 5}", "C2{15, 11, 12, 13, 14, 9, 5}", "C3{15, 6, 7, 8, 9, 10, 5}",
                 "A1 = RS::L1", "L1{15, 0, 1, 11, 12, 13, 14}", "A2{15, 2, 3, 4, 5, 6, 14}", "A3{15, 10, 7, 8, 9, 6, 14}",
                 "B1 = RS::L3F", "L3F{15, 0, 1, 7, 8, 9, 10}", "B2 = RS::L2", "L2{15, 2, 3, 4, 5, 6, 10}",
                 "B3{15, 0, 1, 11, 12, 13, 10}", "B4{15, 0, 1, 14, 11, 12, 10}"):
        assert text in src, text
    lays = {"L3": "{15, 5, 6, 7, 8, 9, 10}", "L4": "{15, 11, 12, 13, 14, 9, 10}", "L5": "{15, 0, 1, 2, 3, 4, 10}",
            "C1": "{15, 0, 1, 2, 3, 4, 5}", "C2": "{15, 11, 12, 13, 14, 9, 5}", "C3": "{15, 6, 7, 8, 9, 10, 5}",
            "A1": "{15, 0, 1, 11, 12, 13, 14}", "A2": "{15, 2, 3, 4, 5, 6, 14}", "A3": "{15, 10, 7, 8, 9, 6, 14}",
            "B1": "{15, 0, 1, 7, 8, 9, 10}", "B2": "{15, 2, 3, 4, 5, 6, 10}", "B3": "{15, 0, 1, 11, 12, 13, 10}",
            "B4": "{15, 0, 1, 14, 11, 12, 10}"}
    for name in PAIRS:
        a, b = name.split()[1].split("->")
        assert '{"%s", %s, %s, ' % (name, lays[a], lays[b]) in chk, name
    used = set(re.findall(r"exchange_half_lin<R::(\w+), R::(\w+),", src))
    assert used == {("L4", "L5"), ("C2", "C3"), ("A1", "A2"), ("B1", "B2"), ("B2", "B3")}
    assert used <= {tuple(n.split()[1].split("->")) for n in PAIRS}


def test_lin_exchange_maps(tmp_path):
    _check_output(subprocess.run([_build(tmp_path, "lds_exchange_check")], capture_output=True, text=True))


def test_lin_exchange_maps_sanitized(tmp_path):
    """The same stand-alone program under AddressSanitizer and UBSan."""
    exe = _build(tmp_path, "lds_exchange_check_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    _check_output(subprocess.run([exe], capture_output=True, text=True))
