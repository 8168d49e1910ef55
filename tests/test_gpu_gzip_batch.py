"""GPU: the batched TLZ gzip (ofl_gzip_ranks_batch, lossy.gzip_ranks_batch, RoundEnd with payloads).  A member's
bytes depend on its values alone: every tensor's payload is lossy.gzip_ranks of its slice, and decompresses to it."""
import ctypes
import gzip

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, M = "cuda:0", 131072                                    # M: values per member
EDGES = [1, 3, 2047, 2048, 2049, M - 1, M, M + 1, 2 * M + 5]  # segment and member edges
CASES = {
    "edges": (EDGES, [sum((n + 63) // 64 * 64 + 64 for n in EDGES[:t]) for t in range(len(EDGES))], 6),
    # members that start 4, 8 and 12 bytes off a 16-byte boundary; 2049 and M + 1 take both load paths in one member
    "unaligned": ([2049, 70, M + 1, 5], [1, 2054, 2127, 2127 + M + 4], 6),
    # 513+ members: two launches, the double buffer, a tail of short members behind two long ones
    "launches": ([70] * 300 + [M + 1] + [70] * 220, [128 * t + (M + 64 if t > 300 else 0) for t in range(521)], 6),
    # a launch whose stream exceeds its staging (1 byte per value) is packed straight into the mapped output.
    # ~300,000 uniform values 0..31 do NOT get there (zlib -9 and TLZ: 0.91 bytes per value, 5 bits of entropy);
    # short tensors do: a member's header and code tables are ~60 bytes whatever it holds
    "over_staging": ([5] * 300, [64 * t for t in range(300)], 32),
}


def _host(name):
    sizes, offs, hi = CASES[name]
    rng = np.random.default_rng(len(sizes))
    host = np.zeros(offs[-1] + sizes[-1] + 3, np.float32)
    for o, n in zip(offs, sizes):       # KC-like: runs of one rank, so copies occur
        host[o:o + n] = np.repeat(rng.integers(0, hi, n), rng.integers(1, 6 if hi == 6 else 2, n))[:n]
    return sizes, offs, host


def _c_batch(x, offs, sizes, cap=None, null=False):
    """The C entry on this thread's workspace -> (rc, payloads, tensor_end)."""
    from openfl_amd import _lib, lossy
    L = _lib.lib()
    off, num = np.asarray(offs, np.int64), np.asarray(sizes, np.int64)
    ws = lossy._ws_bytes(x.device, L.ofl_gzip_ranks_batch_workspace_bytes(len(num), num.ctypes.data))
    cap = L.ofl_gzip_ranks_batch_bound(len(num), num.ctypes.data) if cap is None else cap
    out = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
    ends = np.zeros(len(num), np.uint64)
    rc = L.ofl_gzip_ranks_batch(len(num), x.data_ptr(), None if null else off.ctypes.data, num.ctypes.data, out.data_ptr(),
                                cap, ends.ctypes.data, ws.data_ptr(), ws.numel(), None)
    cuts = [0] + [int(e) for e in ends]
    return rc, [out[a:b].numpy().tobytes() for a, b in zip(cuts, cuts[1:])] if rc == 0 else None, ends


@pytest.mark.parametrize("name", list(CASES))
def test_batch_equals_per_tensor(name):
    from openfl_amd import lossy
    sizes, offs, host = _host(name)
    x = torch.from_numpy(host).to(DEV)
    rc, pay, ends = _c_batch(x, offs, sizes)
    assert rc == 0 and list(np.cumsum([len(p) for p in pay])) == list(ends)
    for o, n, p in zip(offs, sizes, pay):
        assert gzip.decompress(p) == host[o:o + n].tobytes(), (o, n)
        assert p == lossy.gzip_ranks(x[o:o + n]), (o, n)
    assert lossy.gzip_ranks_batch(x, offs, sizes) == pay
    if name == "over_staging":
        assert int(ends[-1]) > (sum(sizes) + 255) // 256 * 256


@pytest.mark.parametrize("bad", ["32", "negative", "fraction", "null_table", "cap_short"])
def test_refusals_then_a_valid_call(bad):
    from openfl_amd import _lib
    sizes, offs, host = _host("unaligned")
    x = torch.from_numpy(host).to(DEV)
    rc, want, ends = _c_batch(x, offs, sizes)
    y = x.clone()
    if bad in ("32", "negative", "fraction"):
        y[offs[2] + M - 1] = {"32": 32.0, "negative": -1.0, "fraction": 2.5}[bad]  # the last value of a full member
    got = _c_batch(y, offs, sizes, cap=int(ends[-1]) - 1 if bad == "cap_short" else None, null=bad == "null_table")[0]
    assert got == (_lib.OFL_ESPACE if bad == "cap_short" else _lib.OFL_EINVAL)
    rc, again, ends2 = _c_batch(x, offs, sizes, cap=int(ends[-1]))                # an exact capacity is enough
    assert rc == 0 and again == want and list(ends2) == list(ends)


@pytest.mark.parametrize("kind", ["kc", "stc"])
def test_round_end_encodes_the_update_in_one_launch(kind):
    from openfl_amd import _lib, pipelines as P
    from openfl_amd.aggregation import RoundEnd
    shapes = [(64, 3, 3, 3), (5,), (65537,), (100,), (1,), (2 * M + 3,)]
    rng = np.random.default_rng(21)
    collabs = [[(rng.standard_normal(s) * 0.01).astype(np.float32) for s in shapes] for _ in range(3)]
    pipe = {"kc": P.KCPipeline, "stc": P.STCPipeline}[kind](p_sparsity=0.1, device=DEV)
    re = RoundEnd(pipe, shapes, DEV)
    L = _lib.lib()
    L.ofl_gzip_profile(1)
    try:
        pay = re.run([re.pack(c) for c in collabs], [0.2, 0.5, 0.3], None, payloads=True)[1]
        names, ms, ln, nk = ctypes.create_string_buffer(4096), np.zeros(16), np.zeros(16, np.int64), ctypes.c_int()
        _lib.check_gzip(L.ofl_gzip_profile_collect(names, 4096, ms.ctypes.data, ln.ctypes.data, 16, ctypes.byref(nk)))
    finally:
        L.ofl_gzip_profile(0)
    launches = dict(zip(names.value.decode().split("\n")[:nk.value], ln.tolist()))
    assert {k: v for k, v in launches.items() if k.startswith("tlz::k_tlz_encode")} == {"tlz::k_tlz_encode<table>": 1}
    for i, s in enumerate(shapes):                          # the batch's bytes are the per-tensor call's
        if int(np.prod(s)) >= (6 if kind == "kc" else 1):   # (the device path's tensors)
            ranks = np.frombuffer(gzip.decompress(pay[i][0]), np.float32).copy()
            assert ranks.size == int(np.prod(s))
            assert pipe.transformers[-1].forward_device(torch.from_numpy(ranks).to(DEV))[0] == pay[i][0], i
