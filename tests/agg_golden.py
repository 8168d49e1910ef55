"""Loader for tests/golden/geometric_median_golden.{npz,json}: the reference's
geometric median on designed cases (tests/golden/make_agg_golden.py; inputs,
weights, float64 results, round counts and the objective after every pass)."""
import json
import os

import numpy as np

from tests.golden_io import GOLDEN


def load():
    arrays = np.load(os.path.join(GOLDEN, "geometric_median_golden.npz"), allow_pickle=False)
    with open(os.path.join(GOLDEN, "geometric_median_golden.json")) as f:
        index = json.load(f)
    return arrays, index


def inputs(arrays, name):
    """The float32 collaborator tensors of a case, decoded exactly as the
    generator fed them to the reference: q * mul[c] + add[c], two float32
    operations per element."""
    q, mul, add = arrays["q_" + name], arrays["mul_" + name], arrays["add_" + name]
    return [q[c].astype(np.float32) * np.float32(mul[c]) + np.float32(add[c]) for c in range(q.shape[0])]
