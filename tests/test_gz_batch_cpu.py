"""The batched gzip encoder's host-only code (gz_members.h: member table, launch
order, sizes) without a GPU: tests/gz_batch_check.cpp, built with ASan and UBSan,
against the rules written out here and the library's workspace size and bound."""
import os
import subprocess

import numpy as np

from tests.test_gz_members_cpu import ROOT, _cxx

M, BATCH = 131072, 512
LISTS = {
    "edges": [(320000 * t + t % 4, n) for t, n in enumerate([1, 3, 2047, 2048, 2049, M - 1, M, M + 1, 2 * M + 5])],
    "launches": [(128 * t + (2 * M if t > 300 else 0), M + 1 if t == 300 else 70 + t % 3) for t in range(521)],
    "empty": [], "empty_tensor": [(0, 5), (64, 0)], "int32_members": [(0, 2 ** 47)] * 3,   # 3 x 2^30 members
}
slot = lambda c: (6 * c + 8192 + 255) // 256 * 256  # noqa: E731


def test_member_table_order_and_sizes(tmp_path):
    from openfl_amd import _lib
    exe = str(tmp_path / "gz_batch_check")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-pthread", "-I", os.path.join(ROOT, "openfl_amd", "csrc"), "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "gz_batch_check.cpp"), "-o", exe], check=True)
    text = "".join(" ".join(f"{o}:{n}" for o, n in lst) + "\n" if lst else "-\n" for lst in LISTS.values())
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    blocks = [b.split("\n") for b in ("\n" + run.stdout.strip()).split("\nL ")[1:]]
    assert len(blocks) == len(LISTS)
    L = _lib.lib()
    for (name, lst), lines in zip(LISTS.items(), blocks):
        num = np.array([n for _, n in lst], np.int64)
        lib = [int(f(len(num), num.ctypes.data)) for f in (L.ofl_gzip_ranks_batch_workspace_bytes, L.ofl_gzip_ranks_batch_bound)]
        head = [int(v) for v in lines[0].split()]
        if name in ("empty", "empty_tensor", "int32_members"):
            assert head[0] == 0 and lines[1] == "P 0" and lib == [0, 0], name
            continue
        recs = [(o + a, min(M, n - a), t) for t, (o, n) in enumerate(lst) for a in range(0, n, M)]
        counts = [c for _, c, _ in recs]
        stage = max(sum(counts[c0:c0 + BATCH]) for c0 in range(0, len(recs), BATCH))
        assert head == [1, len(recs), min(len(recs), BATCH), slot(max(counts)), (max(counts) + 63) // 64 * 64,
                        (stage + 255) // 256 * 256, sum(slot(c) for c in counts)], name
        assert lines[1] == "P 1" and [tuple(int(v) for v in m.split()[1:]) for m in lines if m[0] == "M"] == recs, name
        for o in (m.split() for m in lines if m[0] == "O"):
            part = counts[int(o[1]):int(o[1]) + BATCH]
            assert [int(v) for v in o[2:]] == sorted(range(len(part)), key=lambda j: -part[j]), (name, o[1])  # ties: table order
        for mis, ranks_end, tab, order, tend, end in ([int(v) for v in m.split()[1:]] for m in lines if m[0] == "W"):
            assert ranks_end <= tab and (mis + tab) % 16 == 0 and tab + 16 * len(recs) <= order, (name, mis)
            assert (mis + order) % 4 == 0 and order + 4 * len(recs) <= tend and (mis + tend) % 8 == 0, (name, mis)
            assert tend + 8 * len(lst) <= end == lib[0] and head[6] == lib[1], (name, mis)
