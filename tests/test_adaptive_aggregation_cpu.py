"""No GPU: the adaptive-aggregation fixture (tests/golden/make_adaptive_golden.py)
against a NumPy float32 restatement of the reference's operation sequence.

The GPU tests demand the reference's bits from ofl_adaptive_step.  That is a
fair demand only if the reference's result is a fixed sequence of float32
operations; the restatement below is that sequence written out (every Python
float rounded to float32 once, every operation one float32 NumPy operation,
the gradient summed from +0.0 in collaborator order), and it reproduces the
recorded p, m and v of every case and step byte for byte (NaN where the
reference has NaN).  That also licenses it as the yardstick for the shapes the
fixture does not hold (tests/test_gpu_adaptive_aggregation.py imports it)."""
import os
import re

import numpy as np
import pytest

from tests import adaptive_golden as AG
from tests import golden_io

F = np.float32
DEFAULTS = {"adam": dict(learning_rate=0.01, betas=(0.9, 0.999), initial_accumulator_value=0.0, epsilon=1e-8),
            "yogi": dict(learning_rate=0.01, betas=(0.9, 0.999), initial_accumulator_value=0.0, epsilon=1e-8),
            "adagrad": dict(learning_rate=0.01, initial_accumulator_value=0.1, epsilon=1e-10)}
CASES = {  # name: (collaborators, shape, steps, kinds)
    "default_c3": (3, (4099,), 3, AG.KINDS),
    "custom_c5": (5, (7, 13), 2, AG.KINDS),
    "default_c17": (17, (1027,), 1, AG.KINDS),
    "yogi_negative_v": (3, (257,), 4, ("yogi",)),
    "designed": (3, (37,), 1, AG.KINDS),
}


def restate_gradient(base, xs, weights):
    """AdaptiveAggregation._make_gradient: sum() from int 0 of w * (base - x)."""
    g = np.zeros(np.shape(base), F)  # 0 + first term: +0.0 + t in float32
    for x, w in zip(xs, weights):
        g = g + F(w) * (base - x)
    return g


class Restated:
    """NumPyAdam / NumPyYogi / NumPyAdagrad on one float32 tensor, every
    operation spelled out in float32."""

    def __init__(self, kind, p0, **hyper):
        h = dict(DEFAULTS[kind], **hyper)
        self.kind, self.h, self.t = kind, h, 0
        self.p = np.array(p0, F)
        self.m = np.full_like(self.p, h["initial_accumulator_value"])
        self.v = np.full_like(self.p, h["initial_accumulator_value"])

    def step(self, xs, weights, base):
        h = self.h
        with np.errstate(all="ignore"):
            g = restate_gradient(np.asarray(base, F), [np.asarray(x, F) for x in xs], weights)
            gg = g * g
            lr, eps = F(h["learning_rate"]), F(h["epsilon"])
            if self.kind == "adagrad":
                self.v = self.v + gg
                self.p = self.p - (lr * g) / (np.sqrt(self.v) + eps)
            else:
                b1, b2 = h["betas"]
                t = self.t + 1
                self.m = F(b1) * self.m + F(1.0 - b1) * g
                if self.kind == "yogi":
                    s = np.sign(gg - self.v)
                    self.v = F(b2) * self.v + (F(1.0 - b2) * s) * gg
                else:
                    self.v = F(b2) * self.v + F(1.0 - b2) * gg
                self.p = self.p - (lr * (self.m / F(1.0 - b1 ** t))) / (np.sqrt(self.v / F(1.0 - b2 ** t)) + eps)
            self.t += 1
        assert self.p.dtype == self.v.dtype == self.m.dtype == F
        return self.p.copy()


def assert_same_bits(got, ref, what=""):
    """float32, one shape, NaN in the same places, the same bytes elsewhere."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == F and ref.dtype == F and got.shape == ref.shape, what
    g, r = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(ref).reshape(-1)
    nan = np.isnan(r)
    assert np.array_equal(np.isnan(g), nan), f"{what}: NaN positions differ"
    bad = np.flatnonzero(g.view(np.uint32)[~nan] != r.view(np.uint32)[~nan])
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at {bad[:5]} (of the non-NaN ones)"


def restated_for(arrays, c, kind):
    """A Restated at the start state of a fixture case."""
    _, _, p0 = AG.tensors(arrays, c["name"])
    r = Restated(kind, p0, **AG.hyper(c, kind))
    st = AG.start_state(arrays, c["name"], kind)
    if st is not None:
        m0, v0, t0 = st
        r.v = v0.copy()
        if kind != "adagrad":
            r.m, r.t = m0.copy(), t0
    return r


@pytest.fixture(scope="module")
def golden():
    return AG.load()


def test_fixture_size_shapes_and_dtypes(golden):
    arrays, index = golden
    assert os.path.getsize(AG.NPZ) <= 256 * 1024
    assert {c["name"] for c in index["cases"]} == set(CASES)
    for c in index["cases"]:
        C, shape, steps, kinds = CASES[c["name"]]
        assert (c["C"], tuple(c["shape"]), c["steps"], tuple(c["kinds"])) == (C, shape, steps, tuple(kinds))
        assert c["weights"] == [k / (C * (C + 1) // 2) for k in range(1, C + 1)]   # Python floats k / sum
        x, base, p0 = AG.tensors(arrays, c["name"])
        assert x.dtype == base.dtype == p0.dtype == F
        assert x.shape == (C,) + shape and base.shape == shape and p0.shape == shape
        if c["name"] != "designed":
            assert all(arrays[f"q{k}_{c['name']}"].dtype == np.int8 for k in "xbp")
            assert AG.start_state(arrays, c["name"], kinds[0]) is None
        out = arrays["out_" + c["name"]]
        assert out.dtype == F and out.shape == (len(c["rows"]), int(np.prod(shape)))
        for kind in kinds:
            p, m, v = AG.recorded(arrays, c, kind)
            assert p.shape == (steps,) + shape and v.shape == shape
            assert (m is None) == (kind == "adagrad")
    assert AG.case(index, "default_c3")["hyper"] == {}
    assert AG.hyper(AG.case(index, "custom_c5"), "adam") == dict(
        learning_rate=0.3, betas=(0.5, 0.7), initial_accumulator_value=0.25, epsilon=1e-3)


def test_fixture_edge_cases_are_present(golden):
    arrays, index = golden
    c = AG.case(index, "yogi_negative_v")
    p, _, v = AG.recorded(arrays, c, "yogi")
    assert np.isnan(p).any() and not np.isnan(p[-1]).all()     # the reference itself yields NaN
    assert not np.isnan(p[0]).any()
    d = AG.case(index, "designed")
    x, base, p0 = AG.tensors(arrays, "designed")
    with np.errstate(all="ignore"):
        g = restate_gradient(base, list(x), d["weights"])
        cols = d["columns"]
        assert all(g[k] == 0 and not np.signbit(g[k]) for k in cols["zero_gradient"])
        assert np.signbit(p0[cols["zero_gradient"][0]]) and not np.signbit(p0[cols["zero_gradient"][1]])
        assert all(np.isfinite(g[k]) and abs(g[k]) > 2e38 and np.isinf(g[k] * g[k]) for k in cols["overflow"])
        assert all(0 < g[k] < 1e-43 and g[k] * g[k] == 0 for k in cols["underflow"])
        v0 = AG.start_state(arrays, "designed", "yogi")[1]
        assert all(g[k] * g[k] - v0[k] == 0 and v0[k] > 0 for k in cols["yogi_sign_zero"])
    for r in range(3):   # a NaN in each collaborator, +-inf in one
        assert np.isnan(x[r]).any()
    assert np.isposinf(x).any() and np.isneginf(x).any()
    assert AG.start_state(arrays, "designed", "adam")[2] == 5


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_reference(golden, name):
    arrays, index = golden
    c = AG.case(index, name)
    x, base, _ = AG.tensors(arrays, name)
    for kind in c["kinds"]:
        r = restated_for(arrays, c, kind)
        p_ref, m_ref, v_ref = AG.recorded(arrays, c, kind)
        for s in range(c["steps"]):
            xs, b = AG.step_inputs(x, base, s)
            assert_same_bits(r.step(xs, c["weights"], b), p_ref[s], f"{name}/{kind} p after step {s}")
        assert_same_bits(r.v, v_ref, f"{name}/{kind} v")
        if kind != "adagrad":
            assert_same_bits(r.m, m_ref, f"{name}/{kind} m")


def test_new_symbol_in_header_and_loader():
    from openfl_amd import _lib
    with open(os.path.join(golden_io.GOLDEN, "..", "..", "include", "ofl_codec.h")) as f:
        hdr = f.read()
    assert "ofl_adaptive_step" in set(re.findall(r"\b(ofl_[a-z0-9_]+)\s*\(", hdr))
    assert "ofl_adaptive_step" in _lib.EXPORTS
    assert "ofl_adaptive_consts" in hdr


def test_hyper_parameters_defaults_checks_and_constants():
    """The reference's defaults and ValueErrors (adam_optimizer.py:75-87,
    adagrad_optimizer.py:68-76), and the float32 constants of a step: each
    Python-float expression rounded once."""
    from openfl_amd import aggregation as A
    assert A.ADAPTIVE_AGGREGATIONS == AG.KINDS
    for kind in AG.KINDS:
        h = A.AdaptiveHyper(kind)
        d = DEFAULTS[kind]
        assert (h.learning_rate, h.initial_accumulator_value, h.epsilon) == (
            d["learning_rate"], d["initial_accumulator_value"], d["epsilon"])
        for bad in (dict(learning_rate=-1e-3), dict(initial_accumulator_value=-0.1), dict(epsilon=0.0)):
            with pytest.raises(ValueError):
                A.AdaptiveHyper(kind, **bad)
        A.AdaptiveHyper(kind, learning_rate=0.0)
    for kind in ("adam", "yogi"):
        assert (A.AdaptiveHyper(kind).beta_1, A.AdaptiveHyper(kind).beta_2) == (0.9, 0.999)
        for bad in ((1.0, 0.5), (-0.1, 0.5), (0.5, 1.0), (0.5, -1e-9)):
            with pytest.raises(ValueError):
                A.AdaptiveHyper(kind, betas=bad)
        A.AdaptiveHyper(kind, betas=(0.0, 0.0))
    with pytest.raises(TypeError):
        A.AdaptiveHyper("adagrad", betas=(0.9, 0.999))
    k = A.AdaptiveHyper("yogi", learning_rate=0.3, betas=(0.5, 0.7), epsilon=1e-3).consts(2)
    assert (k.kind, F(k.lr), F(k.beta1), F(k.one_minus_beta1), F(k.beta2), F(k.one_minus_beta2)) == (
        1, F(0.3), F(0.5), F(1.0 - 0.5), F(0.7), F(1.0 - 0.7))
    assert (F(k.bias1), F(k.bias2), F(k.eps)) == (F(1.0 - 0.5 ** 3), F(1.0 - 0.7 ** 3), F(1e-3))
    k = A.AdaptiveHyper("adam").consts(0)
    assert (k.kind, F(k.bias1), F(k.bias2)) == (0, F(1.0 - 0.9), F(1.0 - 0.999))
    k = A.AdaptiveHyper("adagrad").consts(7)
    assert (k.kind, F(k.lr), F(k.eps)) == (2, F(0.01), F(1e-10))
