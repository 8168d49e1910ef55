#!/usr/bin/env python3
"""Generate tests/golden/geometric_median_golden.{npz,json} from the REFERENCE
geometric median.

Test infrastructure, beside make_golden.py and with its rules: it runs only
where the read-only reference checkout is mounted at /root/reference and
refuses to run anywhere else; nothing from the reference is copied, the
fixture holds inputs and recorded outputs only.  The reference's package
``__init__`` chain (dynaconf, ...) is never executed: empty ``openfl``,
``openfl.interface`` and ``openfl.interface.aggregation_functions`` package
objects whose ``__path__`` points into the reference tree are registered first,
with a stub ``...aggregation_functions.core`` that holds a placeholder
``AggregationFunction``.

Reference functions exercised (citations are /root/reference-relative):
  openfl/interface/aggregation_functions/geometric_median.py:13-24  objective
  openfl/interface/aggregation_functions/geometric_median.py:27-56  geometric_median
  openfl/interface/aggregation_functions/geometric_median.py:59-73  _l2dist

The module's _geometric_median_objective is wrapped to record the objective
after every pass; rounds = recorded objectives - 1.

Inputs are stored compactly and exactly: collaborator c of a case is
    x_c = q_c.astype(float32) * mul[c] + add[c]        (two float32 operations)
with q_c int8 (decoded for the tests by tests/agg_golden.py: inputs()).  That
keeps the fixture under 256 KiB; the float64 results are stored in full.

Margin condition (enforced here): in every case whose round count a test
asserts, ratio = |prev - obj| / (ftol * obj) is <= 0.1 or >= 10 at every round,
so a last-bit difference in an objective cannot flip the reference's own break
decision.  obj == 0 (a single collaborator) never breaks whatever the last
bits are and counts as decided (ratio recorded as null).

Usage:  python tests/golden/make_agg_golden.py
"""
import importlib
import json
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
FTOL = 1e-6
MAX_BYTES = 256 * 1024


def _load_reference():
    sub = "openfl/interface/aggregation_functions"
    if not os.path.isfile(os.path.join(REF, sub, "geometric_median.py")):
        sys.exit("make_agg_golden.py: /root/reference is not present; fixtures are generated "
                 "only in the build container")
    for name, path in (("openfl", "openfl"), ("openfl.interface", "openfl/interface"),
                       ("openfl.interface.aggregation_functions", sub)):
        mod = types.ModuleType(name)
        mod.__path__ = [os.path.join(REF, path)]
        sys.modules[name] = mod
    core = types.ModuleType("openfl.interface.aggregation_functions.core")
    core.AggregationFunction = type("AggregationFunction", (), {})
    sys.modules[core.__name__] = core
    return importlib.import_module("openfl.interface.aggregation_functions.geometric_median")


def decode_inputs(q, mul, add):
    return [q[c].astype(np.float32) * np.float32(mul[c]) + np.float32(add[c]) for c in range(q.shape[0])]


def _q(rng, C, shape):
    return np.clip(np.rint(rng.standard_normal((C,) + shape) * 24.0), -127, 127).astype(np.int8)


def cases():
    """(name, q, mul, add, weights, assert_rounds)"""
    out = []
    rng = np.random.default_rng(2024)
    out.append(("c5_shift", _q(rng, 5, (37, 29)), [1 / 24] * 5, [0, 0, 5, 0, 0], [1, 2, 3, 1, 1], True))
    out.append(("c3_small_scale", _q(rng, 3, (1000,)), [0.01 / 24] * 3, [0] * 3, [0.2, 0.5, 0.3], True))
    out.append(("c3_chunks", _q(rng, 3, (12293,)), [1 / 24] * 3, [0] * 3, [1.0, 1.0, 2.0], True))
    w16 = list(np.round(rng.random(16) * 5 + 0.1, 6))
    out.append(("c16_outlier", _q(rng, 16, (2049,)), [1 / 24] * 7 + [30 / 24] + [1 / 24] * 8, [0] * 16, w16, True))
    out.append(("c2_equal_513", _q(rng, 2, (513,)), [1 / 24] * 2, [0] * 2, [1.0, 1.0], True))
    out.append(("c2_equal_1", _q(rng, 2, (1,)), [1 / 24] * 2, [0] * 2, [3.0, 3.0], True))
    out.append(("c1_single", _q(rng, 1, (4097,)), [1 / 24], [0], [2.0], True))
    one = _q(rng, 1, (300,))
    out.append(("c3_identical", np.repeat(one, 3, axis=0), [1 / 24] * 3, [0] * 3, [1.0, 2.0, 3.0], False))
    return out


def main():
    gm = _load_reference()
    record = []
    inner = gm._geometric_median_objective

    def recording(median, tensors, weights):
        v = inner(median, tensors, weights)
        record.append(float(v))
        return v

    gm._geometric_median_objective = recording
    arrays, index = {}, {"ftol": FTOL, "maxiter": 4, "eps": 1e-5, "cases": []}
    for name, q, mul, add, weights, assert_rounds in cases():
        xs = decode_inputs(q, mul, add)
        del record[:]
        with np.errstate(all="ignore"):
            res = gm.geometric_median(np.array(xs), np.array(weights))
        objs = list(record)
        ratios = []
        for prev, obj in zip(objs, objs[1:]):
            ratios.append(None if obj == 0 else abs(prev - obj) / (FTOL * obj))
        if assert_rounds and any(r is not None and 0.1 < r < 10 for r in ratios):
            sys.exit(f"make_agg_golden.py: case {name}: break-test ratio {ratios} within a decade of 1; "
                     "its round count could flip on a last-bit difference")
        assert res.dtype == np.float64 and res.shape == q.shape[1:]
        arrays["q_" + name] = q
        arrays["mul_" + name] = np.asarray(mul, np.float32)
        arrays["add_" + name] = np.asarray(add, np.float32)
        arrays["w_" + name] = np.asarray(weights, np.float64)
        arrays["ref_" + name] = res
        index["cases"].append({"name": name, "C": int(q.shape[0]), "shape": list(q.shape[1:]),
                               "rounds": len(objs) - 1, "objectives": objs, "ratios": ratios,
                               "assert_rounds": assert_rounds})
        print(f"{name}: C={q.shape[0]} shape={q.shape[1:]} rounds={len(objs) - 1} ratios={ratios}")
    path = os.path.join(OUT, "geometric_median_golden.npz")
    np.savez_compressed(path, **arrays)
    with open(os.path.join(OUT, "geometric_median_golden.json"), "w") as f:
        json.dump(index, f, indent=1)
    size = os.path.getsize(path)
    print(f"{path}: {size} bytes")
    if size > MAX_BYTES:
        sys.exit("make_agg_golden.py: the fixture exceeds 256 KiB")


if __name__ == "__main__":
    main()
