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
  --lossy-ingest   instead: one KC-, SKC- and STC-coded upload, ingest()
              against the per-tensor inflate loop it replaced (lossy_ingest).
  --aggregation adam|yogi|adagrad   instead: the FedOpt round end streamed,
              accumulator(base_arena=) + C x add() + finish() against run() on
              the same arenas (12 B per collaborator-element more: the base
              read again and the float32 gradient read and written per add), and ofl_adaptive_accumulate
              and ofl_adaptive_finish alone beside ofl_wavg_accumulate,
              ofl_wavg_finish and k_adaptive in bytes per second (adaptive_stream).
  --upload-stream   instead: the round end from Eden-coded uploads, add_upload x
              C + finish, the decode fused with the accumulate against ingest +
              add, and the last row passes alone (upload_stream).
  --aggregation KIND --upload-stream   instead: that A/B for the FedOpt round,
              the decode fused with the gradient accumulate, k_dec_ada_rowC /
              k_dec_ada_rowC2 beside k_dec_rowC / k_dec_rowC2 + k_adaptive_accumulate
              (upload_stream_adaptive).
  --upload-stream --bf16   instead: that round with a bfloat16 base and model
              against the float32 round on the widened base, same plans, and
              k_dec_acc_rowC2_bf16 / ofl_wavg_finish_bf16 beside their float32
              forms (upload_stream_bf16).
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


def lossy_ingest(args):
    """--lossy-ingest: ingest of one KC-, SKC- and STC-coded upload (the payloads
    of RoundEnd.run) against the per-tensor loop it replaces -- one lut_tables
    H2D and one gunzip_device per tensor, written out below as the parent
    commit had it --, alternated windows; and, with ofl_gzip_profile, the
    kernels on the tensors of at most 2048 values alone: k_tlz_small against
    the k_tlz_ops + k_tlz_resolve pairs."""
    import ctypes
    import torch
    from openfl_amd import _lib, lossy
    from openfl_amd import aggregation as A
    from openfl_amd import pipelines as P
    from openfl_amd.workloads import WORKLOADS
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    shapes = [tuple(s) for _, s in WORKLOADS[args.workload]()]

    def timed(fn, steps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    def kernel_ms(fn):
        """{kernel name: [ms, launches]} of one fn() under ofl_gzip_profile."""
        names, ms, ln, nk = ctypes.create_string_buffer(8192), np.zeros(64), np.zeros(64, np.int64), ctypes.c_int()
        _lib.check_gzip(L.ofl_gzip_profile(1))
        try:
            fn()
            torch.cuda.synchronize()
            _lib.check_gzip(L.ofl_gzip_profile_collect(names, 8192, ms.ctypes.data, ln.ctypes.data, 64, ctypes.byref(nk)))
        finally:
            L.ofl_gzip_profile(0)
        return {k: [round(float(ms[i]), 4), int(ln[i])] for i, k in enumerate(names.value.decode().split("\n")[:nk.value])}

    result = {}
    for name, pipe in (("kc", P.KCPipeline(device=dev)), ("skc", P.SKCPipeline(device=dev)), ("stc", P.STCPipeline(device=dev))):
        re = A.RoundEnd(pipe, shapes, dev)
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        x = torch.empty(re.arena_numel, dtype=torch.float32, device=dev).normal_(0.0, 0.01, generator=g)
        re._zero_gaps(x)
        np.random.seed(0)
        items = re.run([x], [1.0], None, payloads=True)[1]
        out = torch.empty_like(x)
        where = 0 if name == "kc" else 1
        inflated = re._inflated()
        small = [i for i in inflated if re.numels[i] <= 2048]

        def loop(tensors, dst):
            for i in tensors:
                o, n = re.offsets[i], re.numels[i]
                lossy.gunzip_device(items[i][0], dst[o:o + n].view(torch.uint8),
                                    lut=lossy.lut_tables([0], [n], [items[i][1][where]["int_to_float"]], dev),
                                    expect_bytes=4 * n)

        def batch(tensors, dst):
            lossy.gunzip_lut_batch([items[i][0] for i in tensors], [re.offsets[i] for i in tensors],
                                   [re.numels[i] for i in tensors],
                                   [items[i][1][where]["int_to_float"] for i in tensors], dst)

        def parent_ingest():
            dst = re._decode_arena()
            loop(inflated, dst)
            out[:re.arena_numel].copy_(dst)

        def ingest():
            re.ingest(items, delta=False, out=out)

        assert len(inflated) == sum(1 for n in re.numels if n), "a host-path tensor: the parent route below has none"
        parent_ingest()
        want = out.clone()
        ingest()
        same = bool(torch.equal(want.view(torch.int32), out.view(torch.int32)))
        t = {"ingest": [], "parent_loop": []}
        for _ in range(WINDOWS):
            t["ingest"].append(timed(ingest, args.ingest_steps))
            t["parent_loop"].append(timed(parent_ingest, args.ingest_steps))
        dst = re._decode_arena()
        result[name] = {"tensors": len(inflated), "small_tensors": len(small),
                        "wire_bytes": sum(len(p) for p, _ in items), "same_bits": same,
                        "ingest_ms": {"min": round(min(t["ingest"]), 4), "max": round(max(t["ingest"]), 4)},
                        "parent_loop_ms": {"min": round(min(t["parent_loop"]), 4), "max": round(max(t["parent_loop"]), 4)},
                        "kernels_small_tensors": {"batch": kernel_ms(lambda: batch(small, dst)),
                                                  "parent_loop": kernel_ms(lambda: loop(small, dst))},
                        "kernels_all_tensors": {"batch": kernel_ms(lambda: batch(inflated, dst))}}
    print(json.dumps({"metric": "ms, RoundEnd.ingest of one lossy-coded upload (batched inflate) against the per-tensor loop",
                      "workload": args.workload, "windows": WINDOWS, "steps_per_window": args.ingest_steps,
                      "pipelines": result}), flush=True)


def adaptive_stream(args):
    """--aggregation: the streamed FedOpt round end against run(), and the two
    streaming kernels beside their yardsticks, alternated windows in one process."""
    import torch
    from openfl_amd import _lib
    from openfl_amd import aggregation as A
    from openfl_amd.pipelines import EdenPipeline
    from openfl_amd.workloads import WORKLOADS
    dev = torch.device("cuda", 0)
    kind = args.aggregation
    shapes = [tuple(s) for _, s in WORKLOADS[args.workload]()]
    pipe = EdenPipeline(n_bits=8, device=dev, seed_mode="fast")
    re_s, re_r = (A.RoundEnd(pipe, shapes, dev, aggregation=kind) for _ in range(2))
    C, n = args.collaborators, re_s.arena_numel
    g = torch.Generator(device=dev)
    arenas = []
    for c in range(C + 1):
        g.manual_seed(1000 + c)
        a = torch.empty(n, dtype=torch.float32, device=dev).normal_(0.0, 0.01, generator=g)
        re_s._zero_gaps(a)
        arenas.append(a)
    base, collabs = arenas[0], arenas[1:]
    w = [float(v) for v in np.random.default_rng(0).random(C) + 0.5]
    for re in (re_s, re_r):
        re.init_optimizer(base)
    out, grad = torch.empty_like(base), torch.empty_like(base)
    np.random.seed(0)

    def timed(fn, steps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    def windows(fns, steps):
        times = {k: [] for k in fns}
        for _ in range(WINDOWS):
            for k, fn in fns.items():
                times[k].append(timed(fn, steps))
        return times

    def ms(ts):
        return {"min": round(1e3 * min(ts), 4), "max": round(1e3 * max(ts), 4)}

    def stream_round():
        acc = re_s.accumulator(sums=grad, base_arena=base)
        for x, wc in zip(collabs, w):
            acc.add(x, wc)
        re_s.finish(acc, payloads=False, out=out)

    t_round = windows({"streaming": stream_round,
                       "run": lambda: re_r.run(collabs, w, base, payloads=False, out=out)}, args.steps)

    # the kernels alone, by bytes moved, beside the kernels that stream the same arenas
    L = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    hyper, state = re_s._hyper, re_s.optimizer_state()
    p, m, v = state["params"], state["first_moment"], state["second_moment"]
    delta, sums = torch.empty_like(base), torch.empty(n, dtype=torch.float64, device=dev)
    w32 = np.asarray(w, np.float32)
    A.adaptive_accumulate(collabs[0], w32[0], base, n, grad, True, device=dev)
    _lib.check_agg(L.ofl_wavg_accumulate(collabs[0].data_ptr(), 1.0, 1, n, sums.data_ptr(), st))
    sv = 4 if kind == "adagrad" else 0   # adagrad has no first moment: 4 B less each way
    fns = {"adaptive_accumulate_first": lambda: A.adaptive_accumulate(collabs[0], w32[0], base, n, delta, True, device=dev),
           "adaptive_accumulate": lambda: A.adaptive_accumulate(collabs[1 % C], 1e-3, base, n, grad, False, device=dev),
           "adaptive_finish": lambda: A.adaptive_finish(hyper, 0, grad, base, n, p, m, v, delta_out=delta, device=dev),
           "wavg_accumulate": lambda: _lib.check_agg(
               L.ofl_wavg_accumulate(collabs[0].data_ptr(), 1.0, 0, n, sums.data_ptr(), st)),
           "wavg_finish": lambda: _lib.check_agg(
               L.ofl_wavg_finish(sums.data_ptr(), 1.0, base.data_ptr(), n, None, delta.data_ptr(), st)),
           "k_adaptive": lambda: A.adaptive_step(hyper, 0, collabs, w32, base, n, p, m, v, delta_out=delta, device=dev)}
    moved = {"adaptive_accumulate_first": 12 * n, "adaptive_accumulate": 16 * n, "adaptive_finish": (36 - 2 * sv) * n,
             "wavg_accumulate": 20 * n, "wavg_finish": 24 * n, "k_adaptive": (4 * C + 32 - 2 * sv) * n}
    t_k = windows(fns, max(args.steps, 20))
    kernels = {k: {"ms": ms(ts), "bytes_moved": moved[k], "GBps_at_min": round(moved[k] / min(ts) / 1e9, 1),
                   "GBps_at_max": round(moved[k] / max(ts) / 1e9, 1),
                   "frac_of_peak_hbm": round(moved[k] / min(ts) / 1e9 / PEAK_HBM_GBPS, 4)} for k, ts in t_k.items()}
    nbytes = 4 * sum(re_s.numels)
    t = min(t_round["streaming"])
    print(json.dumps({
        "metric": f"GiB/s aggregator round end, {kind} server optimiser, collaborators accumulated one at a time "
                  "(accumulator + C x add + finish: Eden encode/decode + apply), device-resident",
        "value": round(nbytes / t / 2 ** 30, 3), "unit": "GiB/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": ms(t_round["streaming"]), "higher_is_better": True, "dtype": "f32",
        "data": "synthetic N(0, 0.01^2) updates and base, resident in HBM",
        "config": {"workload": args.workload, "tensors": len(shapes), "bytes": nbytes, "collaborators": C,
                   "aggregation": kind, "n_bits": 8, "seed_mode": "fast", "windows": WINDOWS},
        "also": {"run_same_interleave": {"ms_per_step": ms(t_round["run"])},
                 "extra_bytes_streaming": (12 * C - 4) * n,
                 "resident_arena_bytes": {"run": 4 * n * (C + 6 - sv // 4), "streaming": 4 * n * (7 - sv // 4)},
                 "kernels": kernels}}), flush=True)


def upload_stream(args):
    """--upload-stream: the round end fed with Eden-coded uploads, add_upload x
    C + finish, with the decode folded into the sums (fused=True:
    ofl_eden_decode_accumulate) against ingest + add (fused=False), alternated
    windows in one process; then, under the plan's launch events, the last
    row passes alone: k_dec_acc_rowC / k_dec_acc_rowC2 (ws 4 + base 4 + sums
    8 + 8 B per element; the first upload reads no sums) beside k_dec_rowC /
    k_dec_rowC2 (ws 4 + base 4 + y 4) plus ofl_wavg_accumulate (y 4 + sums
    8 + 8), both by bytes over time.  On a commit whose add_upload has no
    fused= the unfused windows run alone, for the parent's figure."""
    import inspect
    import torch
    from openfl_amd import _lib
    from openfl_amd import aggregation as A
    from openfl_amd.pipelines import EdenPipeline
    from openfl_amd.workloads import WORKLOADS
    dev = torch.device("cuda", 0)
    shapes = [tuple(s) for _, s in WORKLOADS[args.workload]()]
    pipe = EdenPipeline(n_bits=8, device=dev, seed_mode="fast")
    re = A.RoundEnd(pipe, shapes, dev)
    C, n = args.collaborators, re.arena_numel
    g = torch.Generator(device=dev)
    arenas = []
    for c in range(C + 1):
        g.manual_seed(1000 + c)
        a = torch.empty(n, dtype=torch.float32, device=dev).normal_(0.0, 0.01, generator=g)
        re._zero_gaps(a)
        arenas.append(a)
    base = arenas[0]
    uploads = [pipe.forward_batch([re.view(a, i).cpu().numpy() for i in range(len(shapes))]) for a in arenas[1:]]
    w = [float(v) for v in np.random.default_rng(0).random(C) + 0.5]
    out = torch.empty_like(base)
    sums = torch.empty(n, dtype=torch.float64, device=dev)
    has_fused = "fused" in inspect.signature(A.WavgAccumulator.add_upload).parameters
    np.random.seed(0)

    def round_end(**kw):
        acc = re.accumulator(sums=sums)
        for items, wc in zip(uploads, w):
            acc.add_upload(items, wc, delta=True, base_arena=base, **kw)
        re.finish(acc, base_arena=base, payloads=False, out=out)
        return acc

    def timed(fn, steps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    fns = {"unfused": lambda: round_end(fused=False), "fused": lambda: round_end(fused=True)} if has_fused \
        else {"unfused_parent": round_end}
    times = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, fn in fns.items():
            times[k].append(timed(fn, args.steps))
    result = {"ms_per_round": {k: {"min": round(min(ts), 4), "max": round(max(ts), 4), "windows": [round(t, 4) for t in ts]}
                               for k, ts in times.items()}}
    if has_fused:
        results = {}
        for k, fn in fns.items():
            np.random.seed(0)   # finish() draws the seeds' offsets
            fn()
            torch.cuda.synchronize()
            results[k] = (sums.clone(), out.clone())
        result["same_bits"] = all(torch.equal(results["fused"][j][o:o + m], results["unfused"][j][o:o + m])
                                  for j in (0, 1) for o, m in zip(re.offsets, re.numels))
        # the last row passes alone: launch events of the plan over `reps` rounds
        p, reps = re.plan, max(args.steps, 10)
        big = sum(ln for t, i in enumerate(re.big) for P, ln in zip(p.dims[t], A.slice_plan(re.numels[i])[1]) if P > 1 << 15)
        rows = {}
        for k, which, rowk in (("unfused", 0, ("ofl::k_dec_rowC", "ofl::k_dec_rowC2")),
                               ("fused", 3, ("ofl::k_dec_acc_rowC", "ofl::k_dec_acc_rowC2"))):
            names = [l["name"] for l in p._launches(which)]
            p.profile(True)
            for _ in range(reps):
                fns[k]()
            torch.cuda.synchronize()
            ms, calls = p.profile_collect(which)
            p.profile(False)
            rows[k] = {"kernels": sorted({nm for nm in names if nm in rowk}), "calls": calls,
                       "ms_per_upload": round(sum(m for m, nm in zip(ms, names) if nm in rowk) / calls, 5)}
        st = torch.cuda.current_stream(dev).cuda_stream
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        acc_ms = []
        for _ in range(reps):
            ev[0].record()
            _lib.check_agg(_lib.lib().ofl_wavg_accumulate(base.data_ptr(), 1.0, 0, n, sums.data_ptr(), st))
            ev[1].record()
            torch.cuda.synchronize()
            acc_ms.append(ev[0].elapsed_time(ev[1]))
        t_acc = min(acc_ms)
        t_un, t_fu = rows["unfused"]["ms_per_upload"], rows["fused"]["ms_per_upload"]
        # per upload, averaged over a round of C: one first upload in C
        b_un_row, b_fu = 12 * big, (24 * (C - 1) + 16) * big / C
        result["row_kernels"] = {
            "large_slice_elements": big, "arena_elements": n,
            "unfused": dict(rows["unfused"], bytes_per_element=12, TBps=round(b_un_row / t_un / 1e9, 3)),
            "wavg_accumulate_whole_arena": {"ms": round(t_acc, 5), "bytes_per_element": 20,
                                            "TBps": round(20 * n / t_acc / 1e9, 3)},
            "unfused_row_plus_accumulate": {"ms": round(t_un + t_acc, 5), "bytes_per_element": 32,
                                            "TBps": round((b_un_row + 20 * n) / (t_un + t_acc) / 1e9, 3)},
            "fused": dict(rows["fused"], bytes_per_element="24 (16 on the first upload of the round)",
                          TBps=round(b_fu / t_fu / 1e9, 3))}
    print(json.dumps({"metric": "ms, round end from Eden-coded uploads: add_upload x C + finish, decode fused with the "
                                "streaming accumulate against ingest + add",
                      "workload": args.workload, "collaborators": C, "windows": WINDOWS, "steps_per_window": args.steps,
                      "warmup": args.warmup, "wire_bytes_per_upload": sum(len(b) for b, _ in uploads[0]), **result}),
          flush=True)


def upload_stream_adaptive(args):
    """--aggregation KIND --upload-stream: the FedOpt round end fed with
    Eden-coded uploads, add_upload x C + finish, with the decode folded into
    the gradient (fused=True: ofl_eden_decode_adaptive_accumulate) against
    ingest + add (fused=False), alternated windows in one process; then, under
    the plan's launch events, the last row passes alone: k_dec_ada_rowC /
    k_dec_ada_rowC2 (ws 4 + base 4 + g 4 + 4 B per element; the first upload
    reads no g) beside k_dec_rowC / k_dec_rowC2 (ws 4 + base 4 + y 4) plus
    k_adaptive_accumulate over the arena (x 4 + base 4 + g 4 + 4), both by
    bytes over time."""
    import torch
    from openfl_amd import aggregation as A
    from openfl_amd.pipelines import EdenPipeline
    from openfl_amd.workloads import WORKLOADS
    dev = torch.device("cuda", 0)
    shapes = [tuple(s) for _, s in WORKLOADS[args.workload]()]
    pipe = EdenPipeline(n_bits=8, device=dev, seed_mode="fast")
    re = A.RoundEnd(pipe, shapes, dev, aggregation=args.aggregation)
    C, n = args.collaborators, re.arena_numel
    g = torch.Generator(device=dev)
    arenas = []
    for c in range(C + 1):
        g.manual_seed(1000 + c)
        a = torch.empty(n, dtype=torch.float32, device=dev).normal_(0.0, 0.01, generator=g)
        re._zero_gaps(a)
        arenas.append(a)
    base = arenas[0]
    re.init_optimizer(base)
    uploads = [pipe.forward_batch([re.view(a, i).cpu().numpy() for i in range(len(shapes))]) for a in arenas[1:]]
    w = [float(v) for v in np.random.default_rng(0).random(C) + 0.5]
    out, grad = torch.empty_like(base), torch.empty_like(base)
    np.random.seed(0)

    def adds(fused):
        acc = re.accumulator(sums=grad, base_arena=base)
        for items, wc in zip(uploads, w):
            acc.add_upload(items, wc, delta=True, base_arena=base, fused=fused)
        return acc

    def timed(fn, steps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    fns = {"unfused": lambda: re.finish(adds(False), payloads=False, out=out),
           "fused": lambda: re.finish(adds(True), payloads=False, out=out)}
    times = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, fn in fns.items():
            times[k].append(timed(fn, args.steps))
    grads = {}
    for k in fns:
        adds(k == "fused")
        torch.cuda.synchronize()
        grads[k] = grad.clone()
    same = all(torch.equal(grads["fused"][o:o + m].view(torch.int32), grads["unfused"][o:o + m].view(torch.int32))
               for o, m in zip(re.offsets, re.numels))
    # the last row passes alone: launch events of the plan over `reps` rounds
    p, reps = re.plan, max(args.steps, 10)
    big = sum(ln for t, i in enumerate(re.big) for P, ln in zip(p.dims[t], A.slice_plan(re.numels[i])[1]) if P > 1 << 15)
    rows = {}
    for k, which, rowk in (("unfused", 0, ("ofl::k_dec_rowC", "ofl::k_dec_rowC2")),
                           ("fused", 7, ("ofl::k_dec_ada_rowC", "ofl::k_dec_ada_rowC2"))):
        names = [l["name"] for l in p._launches(which)]
        p.profile(True)
        for _ in range(reps):
            fns[k]()
        torch.cuda.synchronize()
        ms, calls = p.profile_collect(which)
        p.profile(False)
        rows[k] = {"kernels": sorted({nm for nm in names if nm in rowk}), "calls": calls,
                   "ms_per_upload": round(sum(m for m, nm in zip(ms, names) if nm in rowk) / calls, 5)}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    acc_ms = []
    for _ in range(reps):
        ev[0].record()
        A.adaptive_accumulate(arenas[1], 1e-3, base, n, grad, False, device=dev)
        ev[1].record()
        torch.cuda.synchronize()
        acc_ms.append(ev[0].elapsed_time(ev[1]))
    t_acc = min(acc_ms)
    t_un, t_fu = rows["unfused"]["ms_per_upload"], rows["fused"]["ms_per_upload"]
    # per upload, averaged over a round of C: one first upload in C
    b_un_row, b_fu = 12 * big, (16 * (C - 1) + 12) * big / C
    print(json.dumps({
        "metric": f"ms, {args.aggregation} round end from Eden-coded uploads: add_upload x C + finish, decode fused with "
                  "the gradient accumulate against ingest + add",
        "workload": args.workload, "collaborators": C, "windows": WINDOWS, "steps_per_window": args.steps,
        "warmup": args.warmup, "wire_bytes_per_upload": sum(len(b) for b, _ in uploads[0]), "same_bits": same,
        "ms_per_round": {k: {"min": round(min(ts), 4), "max": round(max(ts), 4), "windows": [round(t, 4) for t in ts]}
                         for k, ts in times.items()},
        "row_kernels": {
            "large_slice_elements": big, "arena_elements": n,
            "unfused": dict(rows["unfused"], bytes_per_element=12, TBps=round(b_un_row / t_un / 1e9, 3)),
            "adaptive_accumulate_whole_arena": {"ms": round(t_acc, 5), "max_ms": round(max(acc_ms), 5),
                                                "bytes_per_element": 16, "TBps": round(16 * n / t_acc / 1e9, 3)},
            "unfused_row_plus_accumulate": {"ms": round(t_un + t_acc, 5), "bytes_per_element": 28,
                                            "TBps": round((b_un_row + 16 * n) / (t_un + t_acc) / 1e9, 3)},
            "fused": dict(rows["fused"], bytes_per_element="16 (12 on the first upload of the round)",
                          TBps=round(b_fu / t_fu / 1e9, 3))}}), flush=True)


def upload_stream_bf16(args):
    """--upload-stream --bf16: add_upload x C + finish with a bfloat16 base and a
    bfloat16 new model against the fused float32 round on the widened base --
    the same RoundEnd, plans, uploads and weights -- in alternated windows of
    one process; then the kernels that differ, alone: the last row passes
    under the plan's launch events (k_dec_acc_rowC / rowC2 against their _bf16
    forms: base 4 -> 2 B per element) and ofl_wavg_finish against
    ofl_wavg_finish_bf16 under device events (24 -> 22 B per element)."""
    import torch
    from openfl_amd import _lib
    from openfl_amd import aggregation as A
    from openfl_amd.pipelines import EdenPipeline
    from openfl_amd.workloads import WORKLOADS
    dev = torch.device("cuda", 0)
    shapes = [tuple(s) for _, s in WORKLOADS[args.workload]()]
    pipe = EdenPipeline(n_bits=8, device=dev, seed_mode="fast")
    re = A.RoundEnd(pipe, shapes, dev)
    C, n = args.collaborators, re.arena_numel
    g = torch.Generator(device=dev)
    arenas = []
    for c in range(C + 1):
        g.manual_seed(1000 + c)
        a = torch.empty(n, dtype=torch.float32, device=dev).normal_(0.0, 0.01, generator=g)
        re._zero_gaps(a)
        arenas.append(a)
    base16 = arenas[0].bfloat16()
    bases = {"f32": base16.float(), "bf16": base16}
    outs = {k: torch.empty_like(b) for k, b in bases.items()}
    uploads = [pipe.forward_batch([re.view(a, i).cpu().numpy() for i in range(len(shapes))]) for a in arenas[1:]]
    w = [float(v) for v in np.random.default_rng(0).random(C) + 0.5]
    sums = torch.empty(n, dtype=torch.float64, device=dev)
    np.random.seed(0)

    def round_end(k):
        acc = re.accumulator(sums=sums)
        for items, wc in zip(uploads, w):
            acc.add_upload(items, wc, delta=True, base_arena=bases[k])
        re.finish(acc, base_arena=bases[k], payloads=False, out=outs[k])

    def timed(fn, steps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    times = {k: [] for k in bases}
    for _ in range(WINDOWS):
        for k in bases:
            times[k].append(timed(lambda: round_end(k), args.steps))
    got = {}
    for k in bases:
        np.random.seed(0)   # finish() draws the seeds' offsets
        round_end(k)
        torch.cuda.synchronize()
        got[k] = sums.clone()
    same = bool(torch.equal(got["f32"].view(torch.int64), got["bf16"].view(torch.int64)) and
                torch.equal(outs["f32"].bfloat16().view(torch.int16), outs["bf16"].view(torch.int16)))
    # the last row passes alone: launch events of the plan over `reps` rounds
    p, reps = re.plan, max(args.steps, 10)
    big = sum(ln for t, i in enumerate(re.big) for P, ln in zip(p.dims[t], A.slice_plan(re.numels[i])[1]) if P > 1 << 15)
    rows = {}
    for k, which in (("f32", 3), ("bf16", 6)):
        names = [l["name"] for l in p._launches(which)]
        p.profile(True)
        for _ in range(reps):
            round_end(k)
        torch.cuda.synchronize()
        ms, calls = p.profile_collect(which)
        p.profile(False)
        b = 2 if k == "bf16" else 4   # per element: ws 4 + base b + sums 8 + 8 (the first upload reads no sums)
        t = sum(m for m, nm in zip(ms, names) if "k_dec_acc_row" in nm) / calls
        rows[k] = {"kernels": sorted({nm for nm in names if "k_dec_acc_row" in nm}), "calls": calls,
                   "ms_per_upload": round(t, 5), "bytes_per_element": f"{20 + b} ({12 + b} on the first upload of the round)",
                   "TBps": round(((20 + b) * (C - 1) + 12 + b) * big / C / t / 1e9, 3)}
    L, st = _lib.lib(), torch.cuda.current_stream(dev).cuda_stream
    delta = torch.empty(n, dtype=torch.float32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fin = {}
    for _ in range(reps):   # alternated
        for k, fn in (("f32", L.ofl_wavg_finish), ("bf16", L.ofl_wavg_finish_bf16)):
            ev[0].record()
            _lib.check_agg(fn(sums.data_ptr(), 1.0, bases[k].data_ptr(), n, None, delta.data_ptr(), st))
            ev[1].record()
            torch.cuda.synchronize()
            fin.setdefault(k, []).append(ev[0].elapsed_time(ev[1]))
    finish = {k: {"ms": {"min": round(min(ts), 5), "max": round(max(ts), 5)}, "bytes_per_element": 22 if k == "bf16" else 24,
                  "TBps_at_min": round((22 if k == "bf16" else 24) * n / min(ts) / 1e9, 3)} for k, ts in fin.items()}
    print(json.dumps({"metric": "ms, round end from Eden-coded uploads (add_upload x C + finish, fused): bfloat16 base and "
                                "model against the float32 round on the widened base",
                      "workload": args.workload, "collaborators": C, "windows": WINDOWS, "steps_per_window": args.steps,
                      "warmup": args.warmup, "same_bits": same, "large_slice_elements": big, "arena_elements": n,
                      "ms_per_round": {k: {"min": round(min(ts), 4), "max": round(max(ts), 4),
                                           "windows": [round(t, 4) for t in ts]} for k, ts in times.items()},
                      "row_kernels": rows, "wavg_finish": finish}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="resnet50_fp32")
    ap.add_argument("--collaborators", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ingest-steps", type=int, default=3)
    ap.add_argument("--lossy-ingest", action="store_true", help="only the KC / SKC / STC ingest A/B")
    ap.add_argument("--aggregation", choices=("adam", "yogi", "adagrad"), help="only the streamed FedOpt round end A/B")
    ap.add_argument("--upload-stream", action="store_true",
                    help="only the upload-streamed round end A/B: add_upload(fused=False | True) x C + finish")
    ap.add_argument("--bf16", action="store_true", help="with --upload-stream: the bfloat16 round against the float32 one")
    args = ap.parse_args()
    if args.lossy_ingest:
        return lossy_ingest(args)
    if args.bf16:
        if not args.upload_stream:
            ap.error("--bf16 goes with --upload-stream")
        return upload_stream_bf16(args)
    if args.upload_stream:
        return upload_stream_adaptive(args) if args.aggregation else upload_stream(args)
    if args.aggregation:
        return adaptive_stream(args)

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
