"""Loader for tests/golden/adaptive_golden.{npz,json}: the reference's
AdaptiveAggregation.call over NumPyAdam / NumPyYogi / NumPyAdagrad on designed
cases (tests/golden/make_adaptive_golden.py; inputs and recorded results only).

A case holds one set of collaborator tensors x[0..C), one base and the starting
parameters, stored as int8 with a float32 scale and offset (the `designed` case:
float32 as they are, it holds NaN, inf and subnormals).  Step s of a case uses
    collaborator c:  x[(c + s) % C]          (the weights stay in place)
    base:            the base rolled by s elements (np.roll of the flat array)
    fl_round:        s  (round 0 looks for the tag "model", later rounds "aggregated")
so every step sees another gradient without another stored tensor.  The
generator feeds the reference through these same functions.

Recorded per optimiser kind K of a case: p after every step (rows "p_K/<step>"
of the float32 array "out_<case>", the row labels in the index), and after the
last step the first moment "m_K" (adam, yogi) and the second moment /
grads_squared "v_K"; recorded() reads them.
"""
import json
import os

import numpy as np

from tests.golden_io import GOLDEN

NPZ = os.path.join(GOLDEN, "adaptive_golden.npz")
KINDS = ("adam", "yogi", "adagrad")


def load():
    arrays = np.load(NPZ, allow_pickle=False)
    with open(os.path.join(GOLDEN, "adaptive_golden.json")) as f:
        index = json.load(f)
    return arrays, index


def case(index, name):
    return next(c for c in index["cases"] if c["name"] == name)


def _decode(arrays, key):
    q = arrays["q" + key]
    if q.dtype == np.float32:
        return q
    mul, add = arrays["mul" + key], arrays["add" + key]
    if mul.ndim == 0:  # one tensor, scalar scale and offset
        return q.astype(np.float32) * mul + add
    return np.stack([q[c].astype(np.float32) * mul[c] + add[c] for c in range(q.shape[0])])


def tensors(arrays, name):
    """-> (x [C, *shape], base [*shape], p0 [*shape]), float32, decoded exactly
    as the generator fed them: q * mul + add, two float32 operations."""
    return _decode(arrays, f"x_{name}"), _decode(arrays, f"b_{name}"), _decode(arrays, f"p_{name}")


def start_state(arrays, name, kind):
    """The designed starting state of a case that has one (else None):
    (m0 or None, v0, steps already taken)."""
    if f"v0_{kind}_{name}" not in arrays:
        return None
    m0 = arrays[f"m0_{kind}_{name}"] if kind != "adagrad" else None
    return m0, arrays[f"v0_{kind}_{name}"], int(arrays[f"t0_{name}"])


def recorded(arrays, c, kind):
    """-> (p after every step [steps, *shape], m after the last or None, v after the last)."""
    out, rows, shape = arrays["out_" + c["name"]], c["rows"], tuple(c["shape"])
    row = lambda k: out[rows.index(k)].reshape(shape)  # noqa: E731
    p = np.stack([row(f"p_{kind}/{s}") for s in range(c["steps"])])
    return p, (row(f"m_{kind}") if kind != "adagrad" else None), row(f"v_{kind}")


def step_inputs(x, base, s):
    """-> (collaborator tensors in order, base) of step s."""
    C = x.shape[0]
    xs = [x[(c + s) % C] for c in range(C)]
    return xs, np.roll(base.reshape(-1), s).reshape(base.shape)


def db_records(tensor_name, fl_round, base):
    """A hand-made db_iterator for AdaptiveAggregation.call: the record it must
    pick is the LAST one of this round and name with the search tag and without
    "delta"; around it, records that differ in exactly one of those."""
    tag = "model" if fl_round == 0 else "aggregated"
    other = "aggregated" if fl_round == 0 else "model"
    wrong = np.full_like(base, 7.0)
    rec = lambda r, n, t, a: {"round": r, "tensor_name": n, "tags": t, "nparray": a}  # noqa: E731
    return [
        rec(fl_round, tensor_name, (tag,), wrong),                # an earlier match: the last one wins
        rec(fl_round, tensor_name, (tag, "extra"), base),         # <- the base
        rec(fl_round, tensor_name, (tag, "delta"), wrong),        # a delta
        rec(fl_round + 1, tensor_name, (tag,), wrong),            # another round
        rec(fl_round, tensor_name + "_", (tag,), wrong),          # another tensor
        rec(fl_round, tensor_name, (other, "trained"), wrong),    # another tag
    ]


def hyper(c, kind):
    """The keyword arguments of a case for one optimiser kind."""
    h = dict(c["hyper"].get(kind, {}))
    if "betas" in h:
        h["betas"] = tuple(h["betas"])
    return h
