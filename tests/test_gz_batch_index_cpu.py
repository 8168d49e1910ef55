"""The batched inflate's member table (gz::inflate_batch_index, gz_members.h)
without a GPU: tests/gz_batch_index_check.cpp runs it on one designed upload,
plain and under ASan + UBSan, on one and three threads.  The reference is
ofl_gzip_member_index of every payload alone: those records, shifted by the
payload's position and its tensor's offset, split at ISIZE 8192, longest first."""
import gzip
import subprocess

import pytest

from tests import bgzf
from tests import gz_members_cases as gc
from tests.test_gz_members_cpu import ROOT, _cxx

OK, NOT_INDEXED, NOT_TLZ, LENGTH = 0, 1, 2, 3


def _upload():
    """(payload, expected decoded bytes, designed verdict) per tensor."""
    m = gc.dc.member_of
    two = m(2049, 1).z + m(100, 2).z                  # the first two-segment member, then a one-segment one
    return [(two, 4 * 2149, OK),
            (m(5000, 3).z, 20000, OK),                # longer: leads the large part
            (m(2048, 4).z, 8192, OK),                 # the last one-segment size
            (gzip.compress(gc.dc.noise(400, 5)), 400, NOT_INDEXED),
            (bgzf.member_indexed(gc.dc.noise(40000, 6)), 40000, NOT_TLZ),
            (m(64, 7).z, 4 * 65, LENGTH),             # the ISIZE sum is not what the caller expects
            (m(5000, 8).z, 20000, OK),                # a tie with payload 1: payload order
            (b"", 0, NOT_INDEXED)]


def _build(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-pthread",
                    "-I", f"{ROOT}/openfl_amd/csrc", "-I", f"{ROOT}/include", f"{ROOT}/tests/gz_batch_index_check.cpp",
                    "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "sanitized"])
@pytest.mark.parametrize("threads", [1, 3])
def test_batch_index_is_the_payloads_indexes_shifted(tmp_path, flags, threads):
    up = _upload()
    pos = [1000 * p + 16 for p in range(len(up))]       # where each payload's copy will stand
    out = [4 * (70000 * p + 3) for p in range(len(up))]  # its tensor's bytes in the arena
    text = "".join(f"{z.hex() or '-'} {pos[p]} {out[p]} {n}\n" for p, (z, n, _) in enumerate(up))
    run = subprocess.run([_build(tmp_path, "check", *flags), str(threads)], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = [ln.split() for ln in run.stdout.splitlines()]
    assert [int(v) for v in lines[0][1:]] == [v for _, _, v in up]
    nlarge, nsmall = int(lines[1][1]), int(lines[1][2])
    got = [tuple(int(w) for w in ln[1:]) for ln in lines if ln[0] == "M"]
    small_payload = [int(v) for v in lines[-1][1:]]
    want_large, want_small = [], []
    for p, (z, _, verdict) in enumerate(up):
        if verdict != OK:
            continue
        alone = gc.library_index(z)
        assert alone["rc"] == 0 and alone["all_tlz"] == 1
        for k in range(alone["n"]):
            w0, w1, w2, w3 = alone["index"][4 * k:4 * k + 4]
            rec = (w0 + pos[p], w1, w2 + out[p], w3)
            (want_large if (w3 & 0xFFFFFFFF) > 8192 else want_small).append((p, rec))
    want_large.sort(key=lambda pr: -(pr[1][3] & 0xFFFFFFFF))   # stable: ties stay in payload and member order
    assert [p for p, _ in want_large] == [1, 6, 0] and [p for p, _ in want_small] == [0, 2]
    assert (nlarge, nsmall) == (3, 2)
    assert got == [r for _, r in want_large + want_small]
    assert small_payload == [p for p, _ in want_small]
