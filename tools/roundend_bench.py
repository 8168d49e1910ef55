#!/usr/bin/env python3
"""Aggregator end of round on the device (openfl_amd.aggregation.RoundEnd).

    python tools/roundend_bench.py [--workload resnet50_fp32] [--collaborators 4] [--steps K]

One step = Aggregator._prepare_trained (aggregator.py:780-865) for every
tensor of the model: np.average over the collaborators' updates, delta to the
previous model, Eden encode + decode of the delta (EdenPipeline, 8 bits, fast
seeds), new model = base + decoded delta.  Collaborator updates and the base
model are resident in HBM; the new model is written to HBM.

Prints one JSON line: value = model GiB per second of round-end work
(fused, device-resident, no payload D2H); also: the unfused sequence
(average kernel writes the delta, the encode reads it), the same with the wire
payloads copied to the host, and the reference's call pattern (per tensor:
host np.average, TensorCodec.generate_delta / compress / decompress /
apply_delta with the openfl_amd EdenPipeline) on the same data.
Roofline: the minimal I/O of the step (read C + 1 fp32 arenas, write one)
against the step time.
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


def robust(args, pipe, shapes, dev, collabs, w, base, out, nbytes, timed):
    """--aggregation median | geometric_median: one JSON line with the round
    end's step time, the aggregation kernels alone (median: bytes moved, 4 C + 4
    + 4 per element with a base; geometric median: all passes of one call and
    the rounds the tensors ran) and the unfused weighted-average round end on
    the same arenas, interleaved."""
    import torch
    from openfl_amd import aggregation as A
    C = len(collabs)
    re = A.RoundEnd(pipe, shapes, dev, aggregation=args.aggregation)
    re_u = A.RoundEnd(pipe, shapes, dev, fused=False)
    t_r, t_u = [], []
    for _ in range(3):
        t_r.append(timed(lambda: re.run(collabs, w, base, payloads=False, out=out), args.steps, args.warmup))
        t_u.append(timed(lambda: re_u.run(collabs, w, base, payloads=False, out=out), args.steps, args.warmup))
    t_pay = timed(lambda: re.run(collabs, w, base, payloads=True, out=out), max(1, args.steps // 2), 1)
    delta = torch.empty(re.arena_numel, dtype=torch.float32, device=dev)
    n = re.arena_numel
    if args.aggregation == "median":
        t_k = timed(lambda: A._median_launch(collabs, base, n, delta=delta, device=dev), args.steps, args.warmup)
        moved = n * (4 * C + 4 + 4)
        kernel = {"kernel": "k_median (median + float32 delta)", "ms": round(1e3 * t_k, 4), "bytes_moved": moved,
                  "GBps": round(moved / t_k / 1e9, 1), "frac_of_peak_hbm": round(moved / t_k / 1e9 / PEAK_HBM_GBPS, 4)}
        w64 = A._f64_weights(w, C)
        wsum = A.weight_sum(w64, 1)
        t_w = timed(lambda: A._wavg_launch(collabs, w64, wsum, base, n, delta32=delta, device=dev),
                    args.steps, args.warmup)
        kernel["k_wavg_delta_same_bytes"] = {"ms": round(1e3 * t_w, 4), "GBps": round(moved / t_w / 1e9, 1)}
    else:
        agg = torch.empty(n, dtype=torch.float64, device=dev)
        w0 = A._gm_start_weights(w, C)
        t_k = timed(lambda: re._gm.launch(collabs, w0, 4, 1e-5, 1e-6, base, agg=agg, delta32=delta, device=dev),
                    args.steps, args.warmup)
        it = re._gm.iters[:len(shapes)].cpu().numpy()
        t_0 = timed(lambda: re._gm.launch(collabs, w0, 0, 1e-5, 1e-6, base, agg=agg, delta32=delta, device=dev),
                    args.steps, args.warmup)
        kernel = {"kernel": "ofl_gmedian_delta (maxiter 4: up to 5 distance passes + the final average)",
                  "ms": round(1e3 * t_k, 4), "ms_maxiter0_one_distance_pass_plus_final": round(1e3 * t_0, 4),
                  "ms_per_extra_round": round(1e3 * (t_k - t_0) / 4, 4),
                  "rounds_min_max": [int(it.min()), int(it.max())],
                  "tensors_by_rounds": {str(k): int((it == k).sum()) for k in sorted(set(it.tolist()))}}
    line = {"metric": f"GiB/s aggregator round end ({args.aggregation} + delta + Eden encode/decode + apply), "
                      "device-resident",
            "value": round(nbytes / min(t_r) / 2 ** 30, 3), "unit": "GiB/s", "n_gpus": 1, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * min(t_r), 3), "higher_is_better": True,
            "dtype": "f32" if args.aggregation == "median" else "f32/f64",
            "data": "synthetic N(0, 0.01^2) updates and base, resident in HBM",
            "config": {"workload": args.workload, "tensors": len(shapes), "bytes": nbytes, "collaborators": C,
                       "n_bits": 8, "seed_mode": args.seed_mode, "aggregation": args.aggregation},
            "also": {"with_payload_d2h": {"ms_per_step": round(1e3 * t_pay, 3)},
                     "unfused_weighted_average_same_interleave": {"ms_per_step": round(1e3 * min(t_u), 3)},
                     "aggregation_alone": kernel}}
    print(json.dumps(line), flush=True)


def adaptive(args, pipe, shapes, dev, collabs, w, base, out, nbytes, timed):
    """--aggregation adam | yogi | adagrad: one JSON line with the round end's
    step time, ofl_adaptive_step alone (with the float32 delta, without agg_out:
    4 C + 16 bytes read and 16 written per element, adagrad 4 C + 12 and 12) and,
    on the same arenas, k_wavg_delta and k_median with their own bytes
    (4 C + 4 read, 4 written) and the unfused weighted-average round end."""
    import torch
    from openfl_amd import aggregation as A
    C = len(collabs)
    w = [float(v) for v in w]   # Python floats, as the aggregator passes them
    re = A.RoundEnd(pipe, shapes, dev, aggregation=args.aggregation)
    re.init_optimizer(base)
    re_u = A.RoundEnd(pipe, shapes, dev, fused=False)
    t_r, t_u = [], []
    for _ in range(3):
        t_r.append(timed(lambda: re.run(collabs, w, base, payloads=False, out=out), args.steps, args.warmup))
        t_u.append(timed(lambda: re_u.run(collabs, w, base, payloads=False, out=out), args.steps, args.warmup))
    t_pay = timed(lambda: re.run(collabs, w, base, payloads=True, out=out), max(1, args.steps // 2), 1)
    n = re.arena_numel
    delta = torch.empty(n, dtype=torch.float32, device=dev)
    st = re.optimizer_state()
    w32 = np.asarray(w, np.float32)
    hyper = A.AdaptiveHyper(args.aggregation)
    t_k = timed(lambda: A.adaptive_step(hyper, 0, collabs, w32, base, n, st["params"], st["first_moment"],
                                        st["second_moment"], delta_out=delta, device=dev), args.steps, args.warmup)
    state = 2 if args.aggregation == "adagrad" else 3
    moved = n * (4 * C + 4 + 8 * state + 4)

    def rate(t, b):
        return {"ms": round(1e3 * t, 4), "bytes_moved": b, "GBps": round(b / t / 1e9, 1),
                "frac_of_peak_hbm": round(b / t / 1e9 / PEAK_HBM_GBPS, 4)}
    kernel = dict({"kernel": "k_adaptive (one optimiser step + float32 delta)"}, **rate(t_k, moved))
    w64 = A._f64_weights(w, C)
    wsum = A.weight_sum(w64, 1)
    small = n * (4 * C + 4 + 4)
    t_w = timed(lambda: A._wavg_launch(collabs, w64, wsum, base, n, delta32=delta, device=dev), args.steps, args.warmup)
    t_m = timed(lambda: A._median_launch(collabs, base, n, delta=delta, device=dev), args.steps, args.warmup)
    kernel["k_wavg_delta"] = rate(t_w, small)
    kernel["k_median"] = rate(t_m, small)
    line = {"metric": f"GiB/s aggregator round end ({args.aggregation} step + delta + Eden encode/decode + apply), "
                      "device-resident",
            "value": round(nbytes / min(t_r) / 2 ** 30, 3), "unit": "GiB/s", "n_gpus": 1, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * min(t_r), 3), "higher_is_better": True,
            "dtype": "f32", "data": "synthetic N(0, 0.01^2) updates and base, resident in HBM",
            "config": {"workload": args.workload, "tensors": len(shapes), "bytes": nbytes, "collaborators": C,
                       "n_bits": 8, "seed_mode": args.seed_mode, "aggregation": args.aggregation},
            "also": {"with_payload_d2h": {"ms_per_step": round(1e3 * t_pay, 3)},
                     "unfused_weighted_average_same_interleave": {"ms_per_step": round(1e3 * min(t_u), 3)},
                     "aggregation_alone": kernel}}
    print(json.dumps(line), flush=True)


def lossy_round(args, shapes, dev, collabs, w, base, out, nbytes, timed):
    """--pipeline kc | skc | stc: one JSON line with the round end's step time
    (RoundEnd with that pipeline, weighted average) in windows alternated with
    -- for kc -- the unfused composition on the same arenas (the same average
    kernel, kmeans_batch with ranks_out, lut_decode_batch, ofl_apply_delta),
    both with and without payloads, and the per-tensor host sequence; and, by
    device events, ofl_label_apply alone (12 B/element) beside the three
    kernels it replaces (28 B/element; k_bkm_label as the difference of a
    k-means with and without ranks_out) and k_wavg_delta."""
    import torch
    from openfl_amd import _lib, lossy
    from openfl_amd import aggregation as A
    from openfl_amd import pipelines as P
    C = len(collabs)
    pipe = {"kc": P.KCPipeline, "skc": P.SKCPipeline, "stc": P.STCPipeline}[args.pipeline](p_sparsity=0.1, device=dev)
    re = A.RoundEnd(pipe, shapes, dev)
    tail = re._tail.__self__
    n, L = re.arena_numel, _lib.lib()
    nel = int(tail.num.sum())
    ranks, dec = torch.empty_like(base), torch.empty_like(base)

    def spread(ts):
        ts = sorted(ts)
        return {"min": round(1e3 * ts[0], 3), "median": round(1e3 * ts[len(ts) // 2], 3), "max": round(1e3 * ts[-1], 3),
                "windows": len(ts)}

    def unfused(payloads):
        delta, _ = re._delta_weighted_average(collabs, w, base, None)
        draws = np.random.randint(0, 2 ** 31 - 1, size=len(tail.dev))
        uniq = lossy.kmeans_batch(delta, tail.off, tail.num, tail.k, n_init=tail.k, seeds=draws, value_f64=True,
                                  ranks_out=ranks)[3]
        maps = [{j: u for j, u in enumerate(uq)} for uq in uniq]
        lossy.lut_decode_batch(ranks, tail.off, tail.num, maps, dec)
        _lib.check_agg(L.ofl_apply_delta(base.data_ptr(), dec.data_ptr(), n, out.data_ptr(), A._stream(dev)))
        if payloads:
            return [tail.gz.forward_device(ranks[o:o + m]) for o, m in zip(tail.off.tolist(), tail.num.tolist())]

    variants = {"round_end": lambda: re.run(collabs, w, base, payloads=False, out=out),
                "round_end_payloads": lambda: re.run(collabs, w, base, payloads=True, out=out)}
    if args.pipeline == "kc":
        variants["unfused"] = lambda: unfused(False)
        variants["unfused_payloads"] = lambda: unfused(True)
    times = {k: [] for k in variants}
    for _ in range(5):
        for k, fn in variants.items():
            pay = k.endswith("payloads")
            times[k].append(timed(fn, max(1, args.steps // 2) if pay else args.steps, 1 if pay else args.warmup))
    also = {k: {"ms_per_step": spread(v)} for k, v in times.items() if k != "round_end"}

    if args.pipeline == "kc":
        delta, _ = re._delta_weighted_average(collabs, w, base, None)
        seeds = np.arange(1, len(tail.dev) + 1)
        vrec = lossy.LabelTable(len(tail.dev), dev)
        km = lambda r, v: lossy.kmeans_batch(delta, tail.off, tail.num, tail.k, n_init=tail.k, seeds=seeds,  # noqa: E731
                                             value_f64=True, ranks_out=r, value_out=v)[3]
        maps = [{j: u for j, u in enumerate(uq)} for uq in km(ranks, vrec)]
        w64 = A._f64_weights(w, C)
        wsum = A.weight_sum(w64, 1)
        kernels = {
            "label_apply": lambda: lossy.label_apply(delta, vrec, base, out),
            "kmeans_with_ranks_out": lambda: km(ranks, None),
            "kmeans_without_ranks_out": lambda: km(None, None),
            "lut_decode_batch": lambda: lossy.lut_decode_batch(ranks, tail.off, tail.num, maps, dec),
            "apply_delta": lambda: L.ofl_apply_delta(base.data_ptr(), dec.data_ptr(), n, out.data_ptr(), A._stream(dev)),
            "wavg_delta": lambda: A._wavg_launch(collabs, w64, wsum, base, n, delta32=dec, device=dev),
        }
        ev = {k: [] for k in kernels}
        for rep in range(args.kernel_reps + 2):
            for k, fn in kernels.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                e.synchronize()
                if rep >= 2:
                    ev[k].append(s.elapsed_time(e) / 1e3)
        med = {k: sorted(v)[len(v) // 2] for k, v in ev.items()}
        label = med["kmeans_with_ranks_out"] - med["kmeans_without_ranks_out"]
        three = label + med["lut_decode_batch"] + med["apply_delta"]

        def rate(t, b):
            return {"ms": round(1e3 * t, 4), "bytes_moved": b, "GBps": round(b / t / 1e9, 1),
                    "frac_of_peak_hbm": round(b / t / 1e9 / PEAK_HBM_GBPS, 4)}
        also["kernels_by_device_events"] = {
            "repetitions": args.kernel_reps, "elements": nel,
            "ofl_label_apply": dict(rate(med["label_apply"], 12 * nel), spread_ms=spread(ev["label_apply"])),
            "three_kernels_it_replaces": dict(rate(three, 28 * nel), parts_ms={
                "k_bkm_label_by_difference": round(1e3 * label, 4),
                "lut_decode_batch_with_its_table_copies": round(1e3 * med["lut_decode_batch"], 4),
                "k_apply": round(1e3 * med["apply_delta"], 4)}),
            "k_wavg_delta": dict(rate(med["wavg_delta"], n * (4 * C + 4 + 4)), spread_ms=spread(ev["wavg_delta"])),
            "kmeans_without_ranks_out_ms": round(1e3 * med["kmeans_without_ranks_out"], 3)}

    if args.host_steps > 0:
        from openfl_amd.tensor_codec import TensorCodec, TensorKey
        tc = TensorCodec(pipe)
        ch = [[re.view(a, i).cpu().numpy() for i in range(len(shapes))] for a in collabs]
        bh = [re.view(base, i).cpu().numpy() for i in range(len(shapes))]
        t0 = time.perf_counter()
        for _ in range(args.host_steps):
            for i in range(len(shapes)):
                agg = np.average([c[i] for c in ch], weights=w, axis=0)
                key = TensorKey(f"t{i}", "aggregator", 0, False, ("aggregated",))
                dk, delta_h = tc.generate_delta(key, agg, bh[i])
                ck, payload, md = tc.compress(dk, delta_h)
                _, dec_h = tc.decompress(ck, payload, md)
                tc.apply_delta(dk, dec_h, bh[i])
        also["per_tensor_reference_call_pattern"] = {
            "ms_per_step": round(1e3 * (time.perf_counter() - t0) / args.host_steps, 1)}
    t = min(times["round_end"])
    line = {"metric": f"GiB/s aggregator round end (average + delta + {args.pipeline.upper()} compress/decompress + "
                      "apply), device-resident",
            "value": round(nbytes / t / 2 ** 30, 3), "unit": "GiB/s", "n_gpus": 1, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": spread(times["round_end"]), "higher_is_better": True,
            "dtype": "f32/f64", "data": "synthetic N(0, 0.01^2) updates and base, resident in HBM",
            "config": {"workload": args.workload, "tensors": len(shapes), "bytes": nbytes, "collaborators": C,
                       "pipeline": args.pipeline, "n_clusters": tail.k, "p_sparsity": 0.1,
                       "host_path_tensors": len(tail.host)},
            "also": also}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="resnet50_fp32")
    ap.add_argument("--collaborators", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed-mode", default="fast")
    ap.add_argument("--host-steps", type=int, default=1, help="steps of the per-tensor host call pattern (0: skip)")
    ap.add_argument("--aggregation", default="weighted_average", choices=["weighted_average", "median", "geometric_median", "adam", "yogi", "adagrad"],
                    help="median / geometric_median / adam / yogi / adagrad: the round end with that aggregator "
                         "(never fused), its aggregation kernels alone, and the unfused weighted-average round "
                         "end beside it")
    ap.add_argument("--pipeline", default="eden", choices=["eden", "kc", "skc", "stc"],
                    help="kc / skc / stc: the round end of that lossy pipeline (weighted average) and, for kc, the "
                         "unfused composition and ofl_label_apply beside the kernels it replaces")
    ap.add_argument("--kernel-reps", type=int, default=20, help="--pipeline kc: device-event repetitions per kernel")
    args = ap.parse_args()

    import torch
    from openfl_amd.aggregation import RoundEnd
    from openfl_amd.pipelines import EdenPipeline
    from openfl_amd.workloads import WORKLOADS
    dev = torch.device("cuda", 0)
    shapes = [tuple(s) for _, s in WORKLOADS[args.workload]()]
    pipe = EdenPipeline(n_bits=8, device=dev, seed_mode=args.seed_mode)
    re = RoundEnd(pipe, shapes, dev)
    C = args.collaborators
    g = torch.Generator(device=dev)
    arenas = []
    for c in range(C + 1):
        g.manual_seed(1000 + c)
        arenas.append(torch.empty(re.arena_numel, dtype=torch.float32, device=dev).normal_(0.0, 0.01, generator=g))
    base, collabs = arenas[0], arenas[1:]
    w = list(np.random.default_rng(0).random(C) + 0.5)
    out = torch.empty_like(base)
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

    if args.pipeline != "eden":
        return lossy_round(args, shapes, dev, collabs, w, base, out, nbytes, timed)
    if args.aggregation in ("adam", "yogi", "adagrad"):
        return adaptive(args, pipe, shapes, dev, collabs, w, base, out, nbytes, timed)
    if args.aggregation != "weighted_average":
        return robust(args, pipe, shapes, dev, collabs, w, base, out, nbytes, timed)

    t_dev = timed(lambda: re.run(collabs, w, base, payloads=False, out=out), args.steps, args.warmup)
    t_pay = timed(lambda: re.run(collabs, w, base, payloads=True, out=out), max(1, args.steps // 2), 1)

    also = {"fused_with_payload_d2h": {"value": round(nbytes / t_pay / 2 ** 30, 3), "ms_per_step": round(1e3 * t_pay, 3)}}
    # A/B: the delta arena written by the averaging kernel and read by the
    # encode (RoundEnd(fused=False)), interleaved with the fused run
    re_u = RoundEnd(pipe, shapes, dev, fused=False)
    t_u, t_f = [], []
    for _ in range(3):
        t_u.append(timed(lambda: re_u.run(collabs, w, base, payloads=False, out=out), args.steps, 1))
        t_f.append(timed(lambda: re.run(collabs, w, base, payloads=False, out=out), args.steps, 1))
    also["unfused_average_then_encode"] = {"value": round(nbytes / min(t_u) / 2 ** 30, 3),
                                           "ms_per_step": round(1e3 * min(t_u), 3),
                                           "fused_same_interleave_ms": round(1e3 * min(t_f), 3)}
    if args.host_steps > 0:
        from openfl_amd.tensor_codec import TensorCodec, TensorKey
        tc = TensorCodec(pipe)
        ch = [[re.view(a, i).cpu().numpy() for i in range(len(shapes))] for a in collabs]
        bh = [re.view(base, i).cpu().numpy() for i in range(len(shapes))]

        def host_round():
            for i in range(len(shapes)):
                agg = np.average([c[i] for c in ch], weights=w, axis=0)
                key = TensorKey(f"t{i}", "aggregator", 0, False, ("aggregated",))
                dk, delta = tc.generate_delta(key, agg, bh[i])
                ck, payload, md = tc.compress(dk, delta)
                _, dec = tc.decompress(ck, payload, md)
                tc.apply_delta(dk, dec, bh[i])
        t0 = time.perf_counter()
        for _ in range(args.host_steps):
            host_round()
        t_host = (time.perf_counter() - t0) / args.host_steps
        also["per_tensor_reference_call_pattern"] = {
            "value": round(nbytes / t_host / 2 ** 30, 4), "ms_per_step": round(1e3 * t_host, 1),
            "note": "host np.average + TensorCodec per tensor, openfl_amd EdenPipeline (GPU codec, one H2D/D2H "
                    "per tensor)"}

    io = 4 * sum(re.numels) * (C + 2)
    line = {"metric": "GiB/s aggregator round end (average + delta + Eden encode/decode + apply), device-resident",
            "value": round(nbytes / t_dev / 2 ** 30, 3), "unit": "GiB/s", "n_gpus": 1, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * t_dev, 3), "higher_is_better": True,
            "dtype": "f32/f64", "data": "synthetic N(0, 0.01^2) updates and base, resident in HBM",
            "config": {"workload": args.workload, "tensors": len(shapes), "bytes": nbytes, "collaborators": C,
                       "n_bits": 8, "seed_mode": args.seed_mode},
            "roofline": {"bound": "hbm", "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                         "achieved": round(io / t_dev / 1e9, 1), "frac": round(io / t_dev / 1e9 / PEAK_HBM_GBPS, 4),
                         "scope": "minimal step I/O: read C updates + base, write the new model (4 B each per "
                                  "element); the codec's own passes come on top", "traffic": None},
            "also": also}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
