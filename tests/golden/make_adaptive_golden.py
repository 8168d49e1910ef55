#!/usr/bin/env python3
"""Generate tests/golden/adaptive_golden.{npz,json} from the REFERENCE
adaptive aggregation (FedOpt server optimisers).

Test infrastructure, beside make_agg_golden.py and with its rules: it runs only
where the read-only reference checkout is mounted at /root/reference and
refuses to run anywhere else; nothing from the reference is copied, the
fixture holds inputs and recorded outputs only.  The reference's package
``__init__`` chain (dynaconf, pandas, ...) is never executed: empty package
objects whose ``__path__`` points into the reference tree are registered for
``openfl``, ``openfl.interface``, ``...aggregation_functions``, ``...core``,
``openfl.utilities``, ``openfl.utilities.optimizers`` and ``...numpy``; a stub
``...core.interface`` holds a placeholder ``AggregationFunction``, and a stub
``openfl.plugins.frameworks_adapters.framework_adapter_interface`` stands in
for base_optimizer's framework import (only model_interface would use it).

Reference code exercised (citations are /root/reference-relative):
  openfl/interface/aggregation_functions/core/adaptive_aggregation.py:38-113
      AdaptiveAggregation._make_gradient, .call
  openfl/utilities/optimizers/numpy/adam_optimizer.py:36-170     NumPyAdam
  openfl/utilities/optimizers/numpy/yogi_optimizer.py:73-94      NumPyYogi
  openfl/utilities/optimizers/numpy/adagrad_optimizer.py:34-124  NumPyAdagrad
  openfl/utilities/types.py  LocalTensor

Every case goes through AdaptiveAggregation.call with the hand-made db_iterator
and the per-step inputs of tests/adaptive_golden.py (db_records, step_inputs).
Recorded: p after every step, m / v (adagrad: grads_squared) after the last,
as the rows of one float32 array per case ("out_<case>", the row labels in the
index: Adam's and Yogi's results are close or equal early on, and side by side
in one deflate stream they cost little more than one of them).
Inputs are stored as int8 with a float32 scale and offset,
    x = q.astype(float32) * mul + add        (two float32 operations)
except the designed case (NaN, inf, subnormals: float32 as they are).  The npz
must stay within 256 KiB.

Usage:  python tests/golden/make_adaptive_golden.py
"""
import importlib
import json
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
MAX_BYTES = 256 * 1024
KINDS = ("adam", "yogi", "adagrad")
NAME = "layer.weight"


def _load_reference():
    if not os.path.isfile(os.path.join(REF, "openfl/interface/aggregation_functions/core/adaptive_aggregation.py")):
        sys.exit("make_adaptive_golden.py: /root/reference is not present; fixtures are generated "
                 "only in the build container")
    for name in ("openfl", "openfl.interface", "openfl.interface.aggregation_functions",
                 "openfl.interface.aggregation_functions.core", "openfl.utilities", "openfl.utilities.optimizers",
                 "openfl.utilities.optimizers.numpy"):
        mod = types.ModuleType(name)
        mod.__path__ = [os.path.join(REF, name.replace(".", "/"))]
        sys.modules[name] = mod
    iface = types.ModuleType("openfl.interface.aggregation_functions.core.interface")

    class AggregationFunction:
        def __call__(self, *args):
            return self.call(*args)

    iface.AggregationFunction = AggregationFunction
    sys.modules[iface.__name__] = iface
    for name in ("openfl.plugins", "openfl.plugins.frameworks_adapters"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod
    fw = types.ModuleType("openfl.plugins.frameworks_adapters.framework_adapter_interface")
    fw.FrameworkAdapterPluginInterface = type("FrameworkAdapterPluginInterface", (), {})
    sys.modules[fw.__name__] = fw
    imp = importlib.import_module
    return {"AdaptiveAggregation": imp("openfl.interface.aggregation_functions.core.adaptive_aggregation").AdaptiveAggregation,
            "adam": imp("openfl.utilities.optimizers.numpy.adam_optimizer").NumPyAdam,
            "yogi": imp("openfl.utilities.optimizers.numpy.yogi_optimizer").NumPyYogi,
            "adagrad": imp("openfl.utilities.optimizers.numpy.adagrad_optimizer").NumPyAdagrad,
            "LocalTensor": imp("openfl.utilities.types").LocalTensor}


def _q(rng, shape, std=24.0):
    return np.clip(np.rint(rng.standard_normal(shape) * std), -127, 127).astype(np.int8)


def _coded(arrays, key, q, mul, add):
    arrays["q" + key] = q
    arrays["mul" + key] = np.asarray(mul, np.float32)
    arrays["add" + key] = np.asarray(add, np.float32)


def random_case(arrays, rng, name, C, shape, scale=0.05):
    adds = [0.01 * (c % 3 - 1) for c in range(C)]
    _coded(arrays, f"x_{name}", _q(rng, (C,) + shape), [scale / 24] * C, adds)
    _coded(arrays, f"b_{name}", _q(rng, shape), scale / 24, 0.0)
    _coded(arrays, f"p_{name}", _q(rng, shape), scale / 24, 0.005)


def designed_case(arrays, ref, name, weights, t0):
    """One step from a designed state; a column is (base, x0, x1, x2, p, m, v)."""
    inf, nan = np.inf, np.nan
    tiny = 12 * 1.401298464324817e-45   # 12 float32 subnormal ulps: g is a few ulps, g * g underflows
    cols = [
        (0.25, 0.25, 0.25, 0.25, -0.0, 0.0, 0.0),          # zero gradient, p = -0.0
        (0.25, 0.25, 0.25, 0.25, 0.0, 0.0, 0.0),           # zero gradient, p = +0.0
        (-1.5, -1.5, -1.5, -1.5, -0.0, 0.125, 0.5),        # zero gradient on a live state
        (3e38, 0.0, 0.0, 0.0, 1.0, 0.5, 0.25),             # g near 3e38: g * g overflows
        (-3e38, 0.0, 0.0, 0.0, 1.0, 0.5, 0.25),
        (tiny, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0),              # g of a few subnormal ulps: g * g underflows
        (tiny, 0.0, 0.0, 0.0, 1e-40, 2e-42, 0.0),
        (0.5, nan, 0.1, 0.2, 1.0, 0.1, 0.2),               # a NaN in each collaborator
        (0.5, 0.1, nan, 0.2, 1.0, 0.1, 0.2),
        (0.5, 0.1, 0.2, nan, 1.0, 0.1, 0.2),
        (0.5, inf, 0.1, 0.2, 1.0, 0.1, 0.2),               # +-inf in one collaborator
        (0.5, 0.1, -inf, 0.2, 1.0, 0.1, 0.2),
        (1.0, 0.5, 0.5, 0.5, 2.0, 0.3, 0.0),               # yogi: v is set to g * g below (sign 0)
        (1.0, 0.5, 0.5, 0.5, 2.0, 0.3, 1.0),               # the same gradient, sign -1
        (1.0, 0.5, 0.5, 0.5, 2.0, 0.3, 1e-3),              # the same gradient, sign +1
        (0.3, 0.1, 0.7, -0.2, -0.4, -0.05, 0.02),          # ordinary columns
        (-0.3, 0.2, 0.1, 0.4, 0.4, 0.05, 0.3),
    ]
    a = np.asarray(cols, np.float32).T
    a = np.concatenate([a, a[:, ::-1], a[:, 5:8]], axis=1)  # 37 columns: the 16-byte body and a tail
    base, x, p, m0, v0 = a[0], a[1:4], a[4], a[5], a[6]
    lts = [ref["LocalTensor"](f"c{c}", x[c], w) for c, w in enumerate(weights)]
    with np.errstate(all="ignore"):
        g = ref["AdaptiveAggregation"]._make_gradient(base, lts)
    assert g.dtype == np.float32
    zero = [12, 2 * len(cols) - 1 - 12]  # column 12 and its mirror image
    for k in zero:
        v0[k] = g[k] * g[k]
        assert g[k] * g[k] - v0[k] == 0 and v0[k] > 0
    arrays[f"qx_{name}"], arrays[f"qb_{name}"], arrays[f"qp_{name}"] = x.copy(), base.copy(), p.copy()
    for kind in KINDS:
        if kind != "adagrad":
            arrays[f"m0_{kind}_{name}"] = m0.copy()
        arrays[f"v0_{kind}_{name}"] = v0.copy()
    arrays[f"t0_{name}"] = np.asarray(t0, np.int64)
    checks = {"zero_gradient": [0, 1, 2], "overflow": [3, 4], "underflow": [5, 6], "yogi_sign_zero": zero}
    with np.errstate(all="ignore"):
        assert all(g[k] == 0 and not np.signbit(g[k]) for k in checks["zero_gradient"])
        assert all(np.isinf(g[k] * g[k]) and np.isfinite(g[k]) for k in checks["overflow"])
        assert all(g[k] != 0 and g[k] * g[k] == 0 for k in checks["underflow"])
    return checks


def _row_order(k):
    """p rows by step, then m, then v; within each the kinds side by side."""
    head, _, step = k.partition("/")
    return head[0] != "p", int(step or 0), head[0], k


def run_case(ref, arrays, c):
    from tests import adaptive_golden as AG
    name = c["name"]
    x, base, p0 = AG.tensors(arrays, name)
    rows = {}
    for kind in c["kinds"]:
        opt = ref[kind](params={NAME: p0.copy()}, **AG.hyper(c, kind))
        st = AG.start_state(arrays, name, kind)
        if st is not None:
            m0, v0, t0 = st
            if kind == "adagrad":
                opt.grads_squared[NAME] = v0.copy()
            else:
                opt.grads_first_moment[NAME] = m0.copy()
                opt.grads_second_moment[NAME] = v0.copy()
                opt.current_step[NAME] = t0
        agg = ref["AdaptiveAggregation"](opt, None)
        ps = []
        for s in range(c["steps"]):
            xs, b = AG.step_inputs(x, base, s)
            lts = [ref["LocalTensor"](f"c{i}", xi, w) for i, (xi, w) in enumerate(zip(xs, c["weights"]))]
            with np.errstate(all="ignore"):
                res = agg.call(lts, AG.db_records(NAME, s, b), NAME, s, ("trained",))
            assert res.dtype == np.float32 and res.shape == p0.shape
            ps.append(res.copy())
        out = {f"p_{kind}/{s}": r for s, r in enumerate(ps)}
        if kind == "adagrad":
            v = opt.grads_squared[NAME]
        else:
            m, v = opt.grads_first_moment[NAME], opt.grads_second_moment[NAME]
            assert m.dtype == np.float32
            out[f"m_{kind}"] = np.asarray(m)
        assert v.dtype == np.float32
        out[f"v_{kind}"] = np.asarray(v)
        rows.update(out)
        nan = int(np.isnan(ps[-1]).sum())
        print(f"{name}/{kind}: C={x.shape[0]} shape={p0.shape} steps={c['steps']} NaN in the last p: {nan}")
    # the same quantity of every kind side by side
    c["rows"] = sorted(rows, key=_row_order)
    arrays[f"out_{name}"] = np.stack([rows[k].reshape(-1) for k in c["rows"]])


def main():
    ref = _load_reference()
    sys.path.insert(0, ROOT)
    rng = np.random.default_rng(2025)
    arrays, cases = {}, []

    def add(name, C, shape, steps, hyper=None, kinds=KINDS):
        cases.append({"name": name, "C": C, "shape": list(shape), "steps": steps, "kinds": list(kinds),
                      "weights": [k / (C * (C + 1) // 2) for k in range(1, C + 1)], "hyper": hyper or {},
                      "tensor_name": NAME})
        return cases[-1]

    random_case(arrays, rng, "default_c3", 3, (4099,))
    add("default_c3", 3, (4099,), 3)
    custom = {"learning_rate": 0.3, "initial_accumulator_value": 0.25, "epsilon": 1e-3}
    random_case(arrays, rng, "custom_c5", 5, (7, 13))
    add("custom_c5", 5, (7, 13), 2, {"adam": dict(custom, betas=[0.5, 0.7]), "yogi": dict(custom, betas=[0.5, 0.7]),
                                     "adagrad": custom})
    random_case(arrays, rng, "default_c17", 17, (1027,))
    add("default_c17", 17, (1027,), 1)
    random_case(arrays, rng, "yogi_negative_v", 3, (257,))
    add("yogi_negative_v", 3, (257,), 4, {"yogi": {"betas": [0.9, 0.3]}}, kinds=("yogi",))
    d = add("designed", 3, (37,), 1)
    d["columns"] = designed_case(arrays, ref, "designed", d["weights"], 5)
    assert d["weights"] == [1 / 6, 2 / 6, 3 / 6]

    for c in cases:
        run_case(ref, arrays, c)
    from tests import adaptive_golden as AG
    p_neg = AG.recorded(arrays, cases[3], "yogi")[0]
    if not np.isnan(p_neg).any():
        sys.exit("make_adaptive_golden.py: yogi_negative_v: no NaN in the recorded p; the case does not "
                 "drive the second moment negative")
    if np.isnan(p_neg).all():
        sys.exit("make_adaptive_golden.py: yogi_negative_v: every element is NaN")
    path = os.path.join(OUT, "adaptive_golden.npz")
    np.savez_compressed(path, **arrays)
    with open(os.path.join(OUT, "adaptive_golden.json"), "w") as f:
        json.dump({"numpy": np.__version__, "cases": cases}, f, indent=1)
    size = os.path.getsize(path)
    print(f"{path}: {size} bytes")
    if size > MAX_BYTES:
        sys.exit("make_adaptive_golden.py: the fixture exceeds 256 KiB")


if __name__ == "__main__":
    main()
