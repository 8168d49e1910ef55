#!/usr/bin/env python3
"""The round end with the collaborators taken one at a time, and the ingest of
one upload, against the routes they replace (openfl_amd.aggregation.RoundEnd).

    python tools/round_stream_bench.py [--workload resnet50_fp32] [--collaborators 4] [--steps K]

One process, windows alternated (A B A B A B, the minimum and the spread of each):
  round end   accumulator() + C x add() + finish() against RoundEnd(fused=False).run()
              on the same resident arenas, payloads=False (Eden, 8 bits, fast
              seeds).  Streaming moves 16 B per collaborator-element more (the
              float64 sums read and written per add), so it is the slower one;
              what it buys is the resident set: 3 arenas and the sums instead
              of C + 3 arenas.
  kernels     ofl_wavg_accumulate (4 + 8 + 8 B/element; the first add 4 + 8)
              against k_wavg_delta (4 C + 4 + 4 B/element) in bytes per second.
  ingest      one Eden-coded upload into an arena: ingest() against
              backward_batch() + pack(), the route through host arrays.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM_GBPS = 8000.0
WINDOWS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="resnet50_fp32")
    ap.add_argument("--collaborators", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ingest-steps", type=int, default=3)
    args = ap.parse_args()

    import torch
    from openfl_amd import _lib
    from openfl_amd import aggregation as A
    from openfl_amd.pipelines import EdenPipeline
    from openfl_amd.workloads import WORKLOADS
    dev = torch.device("cuda", 0)
    shapes = [tuple(s) for _, s in WORKLOADS[args.workload]()]
    pipe = EdenPipeline(n_bits=8, device=dev, seed_mode="fast")
    re = A.RoundEnd(pipe, shapes, dev)
    re_u = A.RoundEnd(pipe, shapes, dev, fused=False)
    C, n = args.collaborators, re.arena_numel
    g = torch.Generator(device=dev)
    arenas = []
    for c in range(C + 1):
        g.manual_seed(1000 + c)
        a = torch.empty(n, dtype=torch.float32, device=dev).normal_(0.0, 0.01, generator=g)
        re._zero_gaps(a)
        arenas.append(a)
    base, collabs = arenas[0], arenas[1:]
    w = [float(v) for v in np.random.default_rng(0).random(C) + 0.5]
    out = torch.empty_like(base)
    sums = torch.empty(n, dtype=torch.float64, device=dev)
    nbytes = 4 * sum(re.numels)
    np.random.seed(0)

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    def windows(fns, steps, warmup):
        """Alternated windows of every fn -> {name: [seconds per step] per window}."""
        times = {k: [] for k in fns}
        for _ in range(WINDOWS):
            for k, fn in fns.items():
                times[k].append(timed(fn, steps, warmup))
        return times

    def ms(ts):
        return {"min": round(1e3 * min(ts), 4), "max": round(1e3 * max(ts), 4)}

    def stream_round():
        acc = re.accumulator(sums=sums)
        for x, wc in zip(collabs, w):
            acc.add(x, wc)
        re.finish(acc, base_arena=base, payloads=False, out=out)

    t_round = windows({"streaming": stream_round,
                       "run_unfused": lambda: re_u.run(collabs, w, base, payloads=False, out=out),
                       "run_fused": lambda: re.run(collabs, w, base, payloads=False, out=out)}, args.steps, args.warmup)

    # the averaging kernels alone, by bytes moved
    L = _lib.lib()
    w64 = A._f64_weights(w, C)
    wsum = A.weight_sum(w64, 1)
    delta = torch.empty(n, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def accumulate_all():
        for c, x in enumerate(collabs):
            _lib.check_agg(L.ofl_wavg_accumulate(x.data_ptr(), float(w64[c]), 1 if c == 0 else 0, n, sums.data_ptr(), st))

    t_k = windows({"accumulate": accumulate_all,
                   "accumulate_not_first": lambda: _lib.check_agg(
                       L.ofl_wavg_accumulate(collabs[0].data_ptr(), 1.0, 0, n, sums.data_ptr(), st)),
                   "finish": lambda: _lib.check_agg(
                       L.ofl_wavg_finish(sums.data_ptr(), wsum, base.data_ptr(), n, None, delta.data_ptr(), st)),
                   "k_wavg_delta": lambda: A._wavg_launch(collabs, w64, wsum, base, n, delta32=delta, device=dev)},
                  max(args.steps, 20), args.warmup)
    moved = {"accumulate": n * (12 + 20 * (C - 1)), "accumulate_not_first": n * 20, "finish": n * 24,
             "k_wavg_delta": n * (4 * C + 8)}
    kernels = {k: {"ms": ms(ts), "bytes_moved": moved[k], "GBps_at_min": round(moved[k] / min(ts) / 1e9, 1),
                   "GBps_at_max": round(moved[k] / max(ts) / 1e9, 1),
                   "frac_of_peak_hbm": round(moved[k] / min(ts) / 1e9 / PEAK_HBM_GBPS, 4)} for k, ts in t_k.items()}

    # one Eden-coded upload: ingest against backward_batch + pack
    host = [re.view(collabs[0], i).cpu().numpy() for i in range(len(shapes))]
    items = pipe.forward_batch(host)
    wire = sum(len(p) for p, _ in items)

    def host_route():
        return re.pack(pipe.backward_batch([(p, list(m)) for p, m in items]))

    def ingest_route():
        return re.ingest(items, delta=False, out=out)

    same = bool(torch.equal(host_route().view(torch.int32), ingest_route().view(torch.int32)))
    t_in = windows({"ingest": ingest_route, "backward_batch_then_pack": host_route}, args.ingest_steps, 1)

    t = min(t_round["streaming"])
    line = {"metric": "GiB/s aggregator round end, collaborators accumulated one at a time (accumulator + C x add + "
                      "finish: Eden encode/decode + apply), device-resident",
            "value": round(nbytes / t / 2 ** 30, 3), "unit": "GiB/s", "n_gpus": 1, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms(t_round["streaming"]), "higher_is_better": True,
            "dtype": "f32/f64", "data": "synthetic N(0, 0.01^2) updates and base, resident in HBM",
            "config": {"workload": args.workload, "tensors": len(shapes), "bytes": nbytes, "collaborators": C,
                       "n_bits": 8, "seed_mode": "fast", "windows": WINDOWS},
            "also": {"run_unfused_same_interleave": {"ms_per_step": ms(t_round["run_unfused"])},
                     "run_fused_same_interleave": {"ms_per_step": ms(t_round["run_fused"])},
                     "resident_arena_bytes": {"run": 4 * n * (C + 3), "streaming": 4 * n * 3 + 8 * n},
                     "kernels": kernels,
                     "ingest_one_upload": {"wire_bytes": wire, "same_bits_as_host_route": same,
                                           "ingest_ms": ms(t_in["ingest"]),
                                           "backward_batch_then_pack_ms": ms(t_in["backward_batch_then_pack"])}}}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
