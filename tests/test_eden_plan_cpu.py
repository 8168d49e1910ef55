"""The Eden planner (openfl_amd/csrc/eden_plan.h) checked on the host:
tests/eden_plan_check.cpp includes the header the library includes, builds the
plans of the designed batches (tests/eden_plan_cases.py) and dumps everything a
plan holds -- layout, launches, what each launch resolves to, the int tables.
The dumps must equal the ones recorded from the commit before the planner
moved into the header (tests/golden/eden_plan_parent.json)."""
import json
import os
import shutil
import subprocess

import pytest

from eden_plan_cases import cases, to_line

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CSRC = os.path.join(ROOT, "openfl_amd", "csrc")
KINDS = ("K_TINY", "K_SMALL", "K_ROWA", "K_ROWC", "K_COL", "K_FINAL", "K_COLM", "K_SSET", "K_COLMSET")
L_FIELDS = ("dir", "idx", "kind", "param", "lo", "mid", "a8", "list_off", "tstart_off", "count", "blocks", "nu", "stream",
            "btab_off", "ptab_off", "npair", "expl", "nt", "sset_off", "sset_groups", "bytes_moved", "bytes_alg")
R_FIELDS = ("ncu", "v", "id", "grid", "tab_off", "npair", "expl", "paired")


def _cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError("no C++ compiler (CXX, c++, g++, clang++)")


def _build(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC,
                    os.path.join(ROOT, "tests", "eden_plan_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe):
    text = "".join(to_line(c) + "\n" for c in cases())
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    kernels, dumps, cur = [], {}, None
    for line in run.stdout.splitlines():
        if line.startswith("K "):
            kernels.append(line)
        elif line.startswith("case "):
            cur = dumps.setdefault(line.split()[1], [])
        else:
            cur.append(line)
    return kernels, dumps


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return _run(_build(tmp_path_factory.mktemp("eden_plan"), "eden_plan_check"))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "eden_plan_parent.json")) as f:
        return json.load(f)


def _launches(lines):
    """-> {'e' / 'd': [(launch fields, [resolve fields])]}, or None where the dump holds a hash."""
    out = {"e": [], "d": []}
    for line in lines:
        f = line.split()
        if f[0] in ("Le#", "Ld#"):
            out[f[0][1]] = None
        elif f[0] == "L":
            out[f[1]].append((dict(zip(L_FIELDS, [f[1]] + [int(v) for v in f[2:]])), []))
            last = out[f[1]][-1]
        elif f[0] == "R":
            last[1].append(dict(zip(R_FIELDS, (int(v) for v in f[1:]))))
    return out


def test_cases_are_the_golden_ones(golden):
    assert [c["name"] for c in cases()] == list(golden["cases"])
    assert len(golden["parent"]) == 40


@pytest.mark.parametrize("name", [c["name"] for c in cases()])
def test_plan_equals_parent(dump, golden, name):
    """Every record of the case's plan, exactly."""
    got, want = dump[1][name], golden["cases"][name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: record {i}"
    assert len(got) == len(want)


def test_kernel_names_equal_parent(dump, golden):
    """The ids of the kernel table and the names reported for them, quirks included."""
    assert dump[0] == golden["kernels"]
    names = [k.split(" ", 2)[2] for k in dump[0]]
    for quirk in ("ofl::k_dec_rowA2", "ofl::k_enc_rowA2", "ofl::k_col6<7, true, 15, true>", "ofl::k_col<5, false>"):
        assert quirk in names
    assert not any("A8" in n or "WAVG" in n for n in names)


def test_cases_reach_every_kind_and_kernel(dump):
    """The ledger: over all cases every launch kind is built and every kernel
    of the table is resolved at least once (in a section written in full)."""
    kinds, ids = set(), set()
    for lines in dump[1].values():
        for sect in _launches(lines).values():
            for l, rs in sect or ():
                kinds.add(l["kind"])
                ids.update(r["id"] for r in rs)
    assert kinds == set(range(len(KINDS)))
    assert ids == set(range(len(dump[0])))


def test_plans_sanitized(tmp_path, dump):
    """The same stand-alone program under AddressSanitizer and UBSan: clean, and the same dump."""
    exe = _build(tmp_path, "eden_plan_check_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert _run(exe) == dump


def test_library_plans_are_the_checkers(dump):
    """The library builds its plans from the header the checker reads: what
    EdenPlan reports equals the checker's dump of the same batch."""
    from openfl_amd.codec import EdenPlan
    names = [k.split(" ", 2)[2] for k in dump[0]]
    for c in cases():
        plan = EdenPlan(c["numels"], c["n_bits"], dims=c["dims"], wave_mib=c["wave_mib"], streams=c["streams"],
                        row2=c["row2"], pair=c["pair"], sset=c["sset"], fuse=c["fuse"])
        lines = dump[1][c["name"]]
        p = [int(v) for v in lines[0].split()[1:]]
        assert (plan.n_waves, plan.planes_bytes, plan.ws_bytes, plan.n_slices) == (p[0], p[3], p[5], p[6]), c["name"]
        for d, sect in _launches(lines).items():
            if sect is None:
                continue
            want = []
            for l, rs in sect:
                r = [r for r in rs if r["ncu"] == 256 and r["v"] == 0][0]   # a plain call before the device is known
                want.append({"name": names[r["id"]], "blocks": l["blocks"], "bytes_moved": l["bytes_moved"],
                             "bytes_alg": l["bytes_alg"], "expl": bool(r["expl"]), "paired": bool(r["paired"]),
                             "grid": r["grid"]})
            assert plan.launches(d == "e") == want, (c["name"], d)
