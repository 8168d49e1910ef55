#!/usr/bin/env python3
"""Eden encode + decode with bfloat16 arenas against float32 arenas, on the
same plans (EdenPlan.encode / decode, ofl_eden_encode_bf16 /
ofl_eden_decode_add_bf16).

    python tools/eden_bf16_ab.py [--workloads uniform_1gib,resnet50_fp32] [--steps K] [--windows N]

One process per run, the two dtypes' windows alternated (A B A B ...; each
window is K encode + decode steps between two device synchronises), the
minimum and the maximum of each.  Then, with the plan's profiling on, the
per-launch times of the first and the last row pass of both dtypes
(profile_collect; events around every launch, so these are not the windows'
times).  The float32 input is the bf16 input widened: both paths encode the
same values; the planes, and y against the float32 y rounded by torch, are
compared once.  Prints one JSON line per
workload.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(workload, steps, windows, bits):
    import torch
    from openfl_amd.codec import EdenPlan
    from openfl_amd.workloads import WORKLOADS, numel
    dev = torch.device("cuda", 0)
    plan = EdenPlan([numel(s) for _, s in WORKLOADS[workload]()], bits)
    n, nt = plan.arena_numel, len(plan.numels)
    g = torch.Generator(device=dev).manual_seed(7)
    x16 = torch.empty(n, device=dev).normal_(0, 0.01, generator=g).bfloat16()
    arenas = {"float32": (x16.float(), torch.empty(n, device=dev)),
              "bfloat16": (x16, torch.empty(n, dtype=torch.bfloat16, device=dev))}
    sd = torch.arange(1, nt + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=dev)
    planes = {k: torch.zeros(max(plan.planes_bytes, 1), dtype=torch.uint8, device=dev) for k in arenas}  # gaps equal
    scales = torch.empty(max(plan.n_slices, 1), device=dev)

    def step(k):
        x, y = arenas[k]
        plan.encode(x, sd, planes[k], scales, ws)
        plan.decode(planes[k], sd, scales, y, ws)

    for k in arenas:   # warm-up: tables to the device, code objects, the side arena
        step(k)
        step(k)
    torch.cuda.synchronize()
    same = bool(torch.equal(planes["float32"], planes["bfloat16"]))
    used = torch.zeros(n, dtype=torch.bool, device=dev)
    for o, m in zip(plan.elem_offsets, plan.numels):
        used[o:o + m] = True
    y_same = bool(torch.equal(arenas["float32"][1].bfloat16().view(torch.int16)[used],
                              arenas["bfloat16"][1].view(torch.int16)[used]))
    del used
    ms = {k: [] for k in arenas}
    for _ in range(windows):
        for k in arenas:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(k)
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0) / steps)
    # the algorithmic bytes of a step: x read, planes written and read, y written
    alg = {"float32": sum(l["bytes_alg"] for d in (True, False) for l in plan.launches(d)),
           "bfloat16": sum(l["bytes_alg"] for d in (True, False) for l in plan.bf16_launches(d))}
    rows = {}
    plan.profile(True)
    for k, (we, wd) in (("float32", (1, 0)), ("bfloat16", (4, 5))):
        for _ in range(steps):
            step(k)
        torch.cuda.synchronize()
        for which, ls, pick in ((we, plan._launches(we), "_rowA"), (wd, plan._launches(wd), "_rowC")):
            t, calls = plan.profile_collect(which)
            for i, l in enumerate(ls):
                if pick in l["name"] and ("enc" in l["name"]) == (which == we):
                    r = rows.setdefault(f"{k} {l['name']}", {"launches": 0, "ms_per_step": 0.0, "bytes_moved": 0})
                    r["launches"] += 1
                    r["ms_per_step"] += float(t[i]) / calls
                    r["bytes_moved"] += l["bytes_moved"]
    plan.profile(False)
    for r in rows.values():
        r["ms_per_step"] = round(r["ms_per_step"], 4)
        r["gbps"] = round(r["bytes_moved"] / r["ms_per_step"] / 1e6, 1)
    return {"workload": workload, "n_bits": bits, "arena_numel": n, "steps_per_window": steps, "planes_equal": same, "y_equal": y_same,
            "alg_bytes_per_step": alg,
            "window_ms": {k: {"min": round(min(v), 4), "max": round(max(v), 4), "all": [round(t, 4) for t in v]}
                          for k, v in ms.items()},
            "row_passes": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="uniform_1gib,resnet50_fp32")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--bits", type=int, default=8)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("eden_bf16_ab.py needs a GPU: a timing on the CPU says nothing")
    for w in args.workloads.split(","):
        print(json.dumps(run(w, args.steps, args.windows, args.bits)), flush=True)


if __name__ == "__main__":
    main()
