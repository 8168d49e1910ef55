"""Designed inputs of tests/test_lossy_layout_cpu.py: arenas for the chunk table
and the workspace layouts of openfl_amd/csrc/lossy_layout.h, the calls the
batched lossy entry points refuse before their first HIP call, and what the
loaded library answers for both (no device: host arrays only, the device
pointers are fake and never followed).

`OFL_CODEC_LIB=<a build of the parent commit> python -m tests.lossy_layout_cases`
prints tests/golden/lossy_layout_parent.json."""
import collections
import json
import sys

import numpy as np

CHUNK = 1 << 16
NUMELS = (1, 5, 65535, 65536, 65537, 2 * 65536 + 17, 1 << 31)
NUMELS_ZERO = (0,) + NUMELS          # zero-length tensors: legal in the LUT and ternary batches only
TS = (1, 2, 3, 64, 65, 4097)
GAPS = (0, 1, 3)
MAX_NK = (0, 1, 6, 64)

Case = collections.namedtuple("Case", "name offsets numels max_nk")


def cases():
    """Every T with every gap, lengths drawn in turn from NUMELS (rotated per
    case, so each T meets each length first) or NUMELS_ZERO, max_nk in turn."""
    out = []
    for draw, tag in ((NUMELS, "n"), (NUMELS_ZERO, "z")):
        for T in TS:
            for gap in GAPS:
                k = len(out)
                num = [draw[(k + t) % len(draw)] for t in range(T)]
                off, at = [], 0
                for n in num:
                    off.append(at)
                    at += n + gap
                out.append(Case(f"{tag}_T{T}_gap{gap}", off, num, MAX_NK[k % len(MAX_NK)]))
    return out


def chunk_table(numels):
    """The restatement the header is checked against: -> (blk0, nblk, blocks)."""
    nblk = [-(-n // CHUNK) for n in numels]
    blk0 = [sum(nblk[:t]) for t in range(len(nblk))] if len(nblk) < 100 else np.concatenate([[0], np.cumsum(nblk)[:-1]]).tolist()
    return blk0, nblk, sum(nblk)


def checker_input():
    return "".join(f"{c.name} {len(c.numels)} {c.max_nk} " + " ".join(f"{o} {n}" for o, n in zip(c.offsets, c.numels)) + "\n"
                   for c in cases())


def library_sizes(c):
    """What the loaded library's *_workspace_bytes report for a case."""
    from openfl_amd import _lib
    L = _lib.lib()
    num = np.asarray(c.numels, np.int64)
    T = len(c.numels)
    return {"kmeans": int(L.ofl_kmeans1d_batch_workspace_bytes(T, num.ctypes.data)),
            "topk": int(L.ofl_sparsify_topk_batch_workspace_bytes(T, num.ctypes.data)),
            "lut": {str(mk): int(L.ofl_lut_decode_batch_workspace_bytes(T, mk)) for mk in MAX_NK},
            "ternary": int(L.ofl_ternary_ranks_batch_workspace_bytes(T)),
            "single": int(L.ofl_lossy_workspace_bytes(int(c.numels[0])))}


X, OUT, WS, TAB = 0x1000, 0x2000, 0x3000, 0x4000   # fake device pointers
BIG = 1 << 40                                      # a workspace size that suffices


def _kmeans_call(fn, **over):
    """ofl_kmeans1d_batch_seeds / _tab with arguments that pass every check up
    to the workspace, then `over` (tests/test_lossy_round_end_cpu.py)."""
    off, num, seeds = np.zeros(1, np.int64), np.full(1, 100, np.int64), np.ones(1, np.uint64)
    a = {"ntensors": 1, "x": X, "off": off.ctypes.data, "num": num.ctypes.data, "k": 6, "seeds": seeds.ctypes.data,
         "label": None, "value": None}
    a.update(over)
    head = (a["ntensors"], a["x"], a["off"], a["num"], a["k"], 6)
    tail = (None, None, None, None, None, None, 0, None)
    if fn == "ofl_kmeans1d_batch_seeds":
        args = head + (a["seeds"], 8, 0, None, a["label"], a["value"]) + tail
    else:
        args = head + (7, 8, 0, None, a["label"]) + tail
    return (off, num, seeds), args


KMEANS_FAULTS = [("no_seeds", {"seeds": None}), ("T0", {"ntensors": 0}), ("Tneg", {"ntensors": -3}), ("no_x", {"x": None}),
                 ("no_off", {"off": None}), ("no_num", {"num": None}), ("k9_value", {"k": 9, "value": TAB}),
                 ("k9_label", {"k": 9, "label": TAB}), ("k0", {"k": 0})]


def _arrays(numels, **more):
    num = np.asarray(numels, np.int64)
    off = np.concatenate([[0], np.cumsum(num)[:-1]]).astype(np.int64)
    return dict(off=off, num=num, **more)


def refusal_calls(L):
    """name -> (function, argument tuple, arrays kept alive): calls the parent
    refuses before its first HIP call without following a pointer it was not
    given (each checked against the parent's code)."""
    calls = {}
    for name, over in KMEANS_FAULTS:
        keep, args = _kmeans_call("ofl_kmeans1d_batch_seeds", **over)
        calls["kmeans_seeds_" + name] = ("ofl_kmeans1d_batch_seeds", args, keep)
        if name == "no_seeds" or "value" in over:
            continue                 # arguments ofl_kmeans1d_batch_tab does not have
        keep, args = _kmeans_call("ofl_kmeans1d_batch_tab", **over)
        calls["kmeans_tab_" + name] = ("ofl_kmeans1d_batch_tab", args, keep)

    def topk(T=1, n=100, k=10, ks=True, short=0):
        a = _arrays([n], ks=np.asarray([k], np.int64))
        need = int(L.ofl_sparsify_topk_batch_workspace_bytes(1, a["num"].ctypes.data)) - 256   # the layout's end
        return ("ofl_sparsify_topk_batch",
                (T, X, a["off"].ctypes.data, a["num"].ctypes.data, a["ks"].ctypes.data if ks else None, OUT, None, None,
                 None, None, None, None, WS, need - short, None), a)
    calls["topk_T0"] = topk(T=0)
    calls["topk_no_ks"] = topk(ks=False)
    calls["topk_k0"] = topk(k=0)
    calls["topk_k_above_n"] = topk(k=101)
    calls["topk_ws_short"] = topk(short=1)

    def lut(T=1, max_nk=6, nk=6, short=0, numels=(100,), off=True, num=True, nks=True):
        a = _arrays(numels, nk=np.full(max(T, 1), nk, np.int32), keys=np.zeros(64, np.float32), vals=np.zeros(64, np.float32))
        need = int(L.ofl_lut_decode_batch_workspace_bytes(T, max_nk))
        return ("ofl_lut_decode_batch",
                (T, X, a["off"].ctypes.data if off else None, a["num"].ctypes.data if num else None,
                 a["nk"].ctypes.data if nks else None, a["keys"].ctypes.data, a["vals"].ctypes.data, max_nk, OUT, WS,
                 need - short, None), a)
    calls["lut_T0"] = lut(T=0)
    calls["lut_max_nk_65"] = lut(max_nk=65)
    calls["lut_ws_short"] = lut(short=1)
    calls["lut_nk_above_max"] = lut(nk=7)

    def ternary(T=1, r3=True, short=0):
        a = _arrays([100], r3=np.zeros(3, np.float32))
        need = int(L.ofl_ternary_ranks_batch_workspace_bytes(T))
        return ("ofl_ternary_ranks_batch",
                (T, X, a["off"].ctypes.data, a["num"].ctypes.data, a["r3"].ctypes.data if r3 else None, OUT, WS,
                 need - short, None), a)
    calls["ternary_T0"] = ternary(T=0)
    calls["ternary_no_ranks3"] = ternary(r3=False)
    calls["ternary_ws_short"] = ternary(short=1)
    # the sanctioned change: refused by the head only (the parent follows the NULL or truncates the grid)
    head_only = {"lut_no_offsets": lut(off=False), "lut_no_numels": lut(num=False), "lut_no_nk": lut(nks=False),
                 "lut_2p47_elements": lut(numels=(1 << 47,)),                   # one tensor too long
                 "lut_2p31_blocks": lut(T=2, numels=(1 << 46, 1 << 46))}        # each legal, 2^31 blocks together
    return calls, head_only


def run_refusals(which=0):
    """name -> [return code, last-error text] from the loaded library."""
    from openfl_amd import _lib
    L = _lib.lib()
    out = {}
    for name, (fn, args, keep) in refusal_calls(L)[which].items():
        rc = getattr(L, fn)(*args)
        out[name] = [int(rc), L.ofl_lossy_last_error().decode()]
        del keep
    return out


if __name__ == "__main__":
    json.dump({"sizes": {c.name: library_sizes(c) for c in cases()}, "refusals": run_refusals()}, sys.stdout, indent=0,
              sort_keys=True)
    sys.stdout.write("\n")
