"""GPU: the FedOpt server optimisers (csrc/agg_kernels.hip: ofl_adaptive_step),
the three plugins and RoundEnd(aggregation="adam" | "yogi" | "adagrad").

Everything is compared bit for bit (NaN in the same places, the same bytes
elsewhere): with the reference's recorded results (tests/golden/
adaptive_golden.*), and for the shapes the fixture does not hold with the
NumPy float32 restatement that tests/test_adaptive_aggregation_cpu.py shows
equal to the reference on every fixture case.  No tolerance is involved: with
float32 parameters and Python-float weights the reference is a fixed sequence
of float32 operations without a reduction, and the kernel performs the same
sequence.  RoundEnd is compared with the reference's per-tensor sequence
(aggregate -> generate_delta -> compress -> decompress -> apply_delta) run
with the same pipeline through the host API."""
import numpy as np
import pytest
import torch

from tests import adaptive_golden as AG
from tests.test_adaptive_aggregation_cpu import CASES, F, Restated, assert_same_bits, restated_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = AG.KINDS
SHAPES = [(), (1,), (2,), (3,), (5,), (7, 13), (1027,), (3, 1, 5), (4099,)]
CUSTOM = {"adam": dict(learning_rate=0.3, betas=(0.5, 0.7), initial_accumulator_value=0.25, epsilon=1e-3),
          "yogi": dict(learning_rate=0.05, betas=(0.8, 0.3), initial_accumulator_value=0.001, epsilon=1e-6),
          "adagrad": dict(learning_rate=0.3, initial_accumulator_value=0.25, epsilon=1e-3)}


def _plugin(kind, **kw):
    from openfl_amd import aggregation as A
    cls = {"adam": A.AdamAdaptiveAggregation, "yogi": A.YogiAdaptiveAggregation,
           "adagrad": A.AdagradAdaptiveAggregation}[kind]
    return cls(device=DEV, **kw)


def _local(xs, weights):
    from openfl_amd.tensor_codec import LocalTensor
    return [LocalTensor(f"c{i}", x, w) for i, (x, w) in enumerate(zip(xs, weights))]


def _weights(C):
    return [k / (C * (C + 1) // 2) for k in range(1, C + 1)]


@pytest.fixture(scope="module")
def golden():
    return AG.load()


# ------------------------------------------------ plugins against the fixture ---
@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(CASES) for k in CASES[n][3]])
def test_plugin_equals_the_reference(golden, name, kind):
    arrays, index = golden
    c = AG.case(index, name)
    tn = c["tensor_name"]
    x, base, p0 = AG.tensors(arrays, name)
    plug = _plugin(kind, params={tn: p0.copy()}, **AG.hyper(c, kind))
    st = AG.start_state(arrays, name, kind)
    if st is not None:
        plug.set_state(tn, first_moment=st[0], second_moment=st[1], step=st[2] if kind != "adagrad" else None)
    p_ref, m_ref, v_ref = AG.recorded(arrays, c, kind)
    for s in range(c["steps"]):
        xs, b = AG.step_inputs(x, base, s)
        got = plug.call(_local(xs, c["weights"]), AG.db_records(tn, s, b), tn, s, ("trained",))
        assert_same_bits(got, p_ref[s], f"{name}/{kind} p after step {s}")
    state = plug.state(tn)
    assert state["step"] == c["steps"] + (st[2] if st is not None and kind != "adagrad" else 0)
    assert_same_bits(state["params"], p_ref[-1], f"{name}/{kind} device p")
    assert_same_bits(state["second_moment"], v_ref, f"{name}/{kind} device v")
    if kind != "adagrad":
        assert_same_bits(state["first_moment"], m_ref, f"{name}/{kind} device m")
    else:
        assert state["first_moment"] is None
    assert p0.tobytes() == AG.tensors(arrays, name)[2].tobytes()   # the caller's array is not touched


# ------------------------------------------ shape sweep against the restatement ---
@pytest.mark.parametrize("C", [1, 2, 3, 4, 16, 17, 33])
def test_plugin_shapes_and_collaborator_counts(C):
    """The 16-byte body and the scalar tail, the unrolled path (C <= 16) and the
    table path (C > 16); default and non-default hyper-parameters, two steps."""
    w = _weights(C)
    for si, shape in enumerate(SHAPES):
        for kind in KINDS:
            hyper = CUSTOM[kind] if si % 2 else {}
            rng = np.random.default_rng(1000 * C + 10 * si + KINDS.index(kind))
            p0 = (rng.standard_normal(shape) * 0.1).astype(F)
            plug = _plugin(kind, params={"t": p0.copy()}, **hyper)
            r = Restated(kind, p0, **hyper)
            for s in range(2):
                base = np.asarray(rng.standard_normal(shape) * 0.1).astype(F)
                xs = [np.asarray(base + rng.standard_normal(shape) * 0.02).astype(F) for _ in range(C)]
                got = plug(_local(xs, w), AG.db_records("t", s, base), "t", s, ("trained",))
                what = f"C={C} {shape} {kind} step {s}"
                assert got.shape == shape
                assert_same_bits(got, r.step(xs, w, base).reshape(shape), what + " p")
            state = plug.state("t")
            assert_same_bits(state["second_moment"], r.v.reshape(shape), what + " v")
            if kind != "adagrad":
                assert_same_bits(state["first_moment"], r.m.reshape(shape), what + " m")


@pytest.mark.parametrize("C", [3, 17])
@pytest.mark.parametrize("offset", [0, 1])
def test_step_on_arena_views(C, offset):
    """adaptive_step on views of larger device arenas: offset 0 is 16-byte
    aligned (the vector body), offset 1 is not (every element through the scalar
    path); agg_out and delta_out, and nothing written outside the n elements."""
    from openfl_amd import aggregation as A
    w = _weights(C)
    w32 = np.asarray(w, F)
    for n in (5, 1027, 4099):
        for kind in KINDS:
            rng = np.random.default_rng(n + C)
            r = Restated(kind, (rng.standard_normal(n) * 0.1).astype(F), **CUSTOM[kind])
            base = (rng.standard_normal(n) * 0.1).astype(F)
            xs = [(base + rng.standard_normal(n) * 0.02).astype(F) for _ in range(C)]

            def arena(a):
                t = torch.full((n + offset + 3,), 9.0, dtype=torch.float32, device=DEV)
                t[offset:offset + n] = torch.from_numpy(a).to(DEV)
                return t
            ax, ab = [arena(x) for x in xs], arena(base)
            ap, am, av = arena(r.p), arena(r.m), arena(r.v)
            agg, delta = arena(np.zeros(n, F)), arena(np.zeros(n, F))
            view = lambda t: t[offset:offset + n]  # noqa: E731
            assert view(ap).data_ptr() % 16 == 4 * offset
            A.adaptive_step(A.AdaptiveHyper(kind, **CUSTOM[kind]), 0, [view(t) for t in ax], w32, view(ab), n,
                            view(ap), view(am) if kind != "adagrad" else None, view(av),
                            agg_out=view(agg), delta_out=view(delta), device=DEV)
            p = r.step(xs, w, base)
            what = f"C={C} n={n} {kind} offset {offset}"
            assert_same_bits(view(ap).cpu().numpy(), p, what + " p")
            assert_same_bits(view(agg).cpu().numpy(), p, what + " agg_out")
            assert_same_bits(view(delta).cpu().numpy(), p - base, what + " delta_out")
            assert_same_bits(view(av).cpu().numpy(), r.v, what + " v")
            if kind != "adagrad":
                assert_same_bits(view(am).cpu().numpy(), r.m, what + " m")
            for t in (ap, av, agg, delta):   # the elements around the view are untouched
                assert bool((t[:offset] == 9.0).all()) and bool((t[offset + n:] == 9.0).all()), what


# ----------------------------------------------- default aggregation and errors ---
def test_default_aggregation_and_errors():
    from openfl_amd import _lib
    from openfl_amd import aggregation as A
    rng = np.random.default_rng(4)
    x = [rng.standard_normal(9).astype(F) for _ in range(3)]
    base = rng.standard_normal(9).astype(F)
    w = _weights(3)
    plug = _plugin("adam", params={"in": base.copy()})
    # a name the optimiser does not own goes to agg_func (default: the weighted average)
    got = plug.call(_local(x, w), [], "other", 0, ("trained",))
    assert got.dtype == np.float64 and got.tobytes() == np.average(x, weights=w, axis=0).tobytes()
    assert _plugin("yogi", params={"in": base.copy()}, agg_func=A.Median(DEV)).call(
        _local(x, w), [], "other", 0, ()).tobytes() == np.median(np.array(x), axis=0).tobytes()
    assert plug.state("in")["step"] == 0
    # no base record of this round / tag / name, or only a delta
    for recs in ([], AG.db_records("in", 1, base), AG.db_records("other", 0, base),
                 [{"round": 0, "tensor_name": "in", "tags": ("model", "delta"), "nparray": base}]):
        with pytest.raises(KeyError):
            plug.call(_local(x, w), recs, "in", 0, ("trained",))
    recs = AG.db_records("in", 0, base)
    with pytest.raises(_lib.CodecError, match="float64"):
        plug.call(_local(x, [np.float64(v) for v in w]), recs, "in", 0, ())
    with pytest.raises(_lib.CodecError):
        plug.call(_local(x, [np.float16(v) for v in w]), recs, "in", 0, ())
    with pytest.raises(_lib.CodecError):
        plug.call([], recs, "in", 0, ())
    with pytest.raises(_lib.CodecError):
        plug.call(_local([x[0], x[1].astype(np.float64), x[2]], w), recs, "in", 0, ())
    with pytest.raises(_lib.CodecError):
        plug.call(_local([x[0], x[1][:5], x[2]], w), recs, "in", 0, ())
    assert plug.state("in")["step"] == 0 and plug.state("in")["params"].tobytes() == base.tobytes()
    # np.float32 weights are what a Python float becomes: the same result; a Python int too
    a = _plugin("adam", params={"in": base.copy()}).call(_local(x, w), recs, "in", 0, ())
    b = _plugin("adam", params={"in": base.copy()}).call(_local(x, [F(v) for v in w]), recs, "in", 0, ())
    assert a.tobytes() == b.tobytes()
    c = _plugin("adagrad", params={"in": base.copy()}).call(_local(x, [1, 2, 3]), recs, "in", 0, ())
    assert_same_bits(c, Restated("adagrad", base).step(x, [1, 2, 3], base))
    for kind in KINDS:
        for bad in (dict(learning_rate=-1.0), dict(initial_accumulator_value=-1.0), dict(epsilon=0.0)):
            with pytest.raises(ValueError):
                _plugin(kind, params={"in": base.copy()}, **bad)
    for kind in ("adam", "yogi"):
        for bad in ((1.0, 0.5), (0.5, 1.0), (-0.1, 0.5)):
            with pytest.raises(ValueError):
                _plugin(kind, params={"in": base.copy()}, betas=bad)
    with pytest.raises(ValueError):
        _plugin("adam", params=None)
    with pytest.raises(_lib.CodecError):
        _plugin("adam", params={"in": base.astype(np.float64)})


def test_collaborator_limit():
    from openfl_amd import _lib
    from openfl_amd import aggregation as A
    rng = np.random.default_rng(8)
    base = rng.standard_normal(70).astype(F)
    xs = [(base + rng.standard_normal(70) * 0.1).astype(F) for _ in range(129)]
    recs = AG.db_records("in", 0, base)
    w = [1.0 / 129] * 129
    with pytest.raises(_lib.CodecError, match="128"):
        _plugin("adam", params={"in": base.copy()}).call(_local(xs, w), recs, "in", 0, ())
    # the limit is the library's own, too
    t = torch.ones(8, dtype=torch.float32, device=DEV)
    ptrs = np.asarray([t.data_ptr()] * 129, np.uint64)
    w32 = np.ones(129, F)
    k = A.AdaptiveHyper("adam").consts(0)
    import ctypes
    rc = _lib.lib().ofl_adaptive_step(129, ptrs.ctypes.data, w32.ctypes.data, t.data_ptr(), 8, t.data_ptr(),
                                      t.data_ptr(), t.data_ptr(), ctypes.addressof(k), None, None,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.OFL_EINVAL and b"128" in _lib.lib().ofl_agg_last_error()
    torch.cuda.synchronize()
    assert bool((t == 1.0).all())
    for kind in KINDS:
        got = _plugin(kind, params={"in": base.copy()}).call(_local(xs[:128], w[:128]), recs, "in", 0, ())
        assert_same_bits(got, Restated(kind, base).step(xs[:128], w[:128], base), f"128 collaborators, {kind}")


# ---------------------------------------------------------------- RoundEnd ---
RE_SHAPES = [(64, 3, 3, 3), (64,), (1,), (300, 200), (5000,), (2, 2), (70_001,), (100,), (101,)]


def _reference_round(pipe, shapes, aggs, base):
    """_prepare_trained per tensor with the host API, from the aggregate on:
    generate_delta -> compress -> decompress -> apply_delta."""
    from openfl_amd.tensor_codec import TensorCodec, TensorKey
    tc = TensorCodec(pipe)
    payloads, models = [], []
    for i, s in enumerate(shapes):
        key = TensorKey(f"t{i}", "aggregator_x", 0, False, ("aggregated",))
        dk, delta = tc.generate_delta(key, aggs[i], base[i])
        ck, payload, md = tc.compress(dk, delta)
        payloads.append((payload, [dict(m) for m in md]))
        _, dec = tc.decompress(ck, payload, md)
        _, new = tc.apply_delta(dk, dec, base[i])
        models.append(np.asarray(new, np.float32).reshape(s))
    return payloads, models


def _seeds_of(payloads, numels, threshold):
    return [int(md[0]["int_to_float"][0]) for (_, md), n in zip(payloads, numels) if n > threshold]


@pytest.mark.parametrize("seed_mode", ["fast", "reference"])
@pytest.mark.parametrize("kind", KINDS)
def test_round_end_matches_per_tensor(kind, seed_mode):
    from openfl_amd import _lib
    from openfl_amd.aggregation import RoundEnd
    from openfl_amd.pipelines import EdenPipeline
    C, shapes = 3, RE_SHAPES
    w = _weights(C)
    # adam: the defaults; betas[1] >= 0.5 keeps yogi's second moment >= 0, so no NaN reaches the
    # seed formula (CPython's hash of a NaN is an object id, which nothing can reproduce)
    hyper = {"adam": {}, "yogi": dict(learning_rate=0.02, betas=(0.8, 0.95), initial_accumulator_value=0.01,
                                      epsilon=1e-6),
             "adagrad": dict(learning_rate=0.02, initial_accumulator_value=0.25, epsilon=1e-3)}[kind]
    rng = np.random.default_rng(50 + KINDS.index(kind))
    params = [(rng.standard_normal(s) * 0.1).astype(F) for s in shapes]
    base = [(p + rng.standard_normal(p.shape) * 0.01).astype(F) for p in params]
    pipe = EdenPipeline(n_bits=8, device=DEV, seed_mode=seed_mode)
    re = RoundEnd(pipe, shapes, DEV, aggregation=kind, optimizer=hyper)
    assert not re.fused
    big = [i for i, n in enumerate(re.numels) if n > re.dim_threshold]
    arenas0 = [re.pack([np.zeros(s, F) for s in shapes])] * C
    with pytest.raises(_lib.CodecError):     # no state yet
        re.run(arenas0, w, re.pack(base))
    with pytest.raises(_lib.CodecError):
        re.optimizer_state()
    re.init_optimizer(re.pack(params))
    with pytest.raises(_lib.CodecError):     # the gradient needs the base
        re.run(arenas0, w, None)
    with pytest.raises(_lib.CodecError):     # the aggregate is float32
        re.run(arenas0, w, re.pack(base), agg_out=torch.empty(re.arena_numel, dtype=torch.float64, device=DEV))
    with pytest.raises(_lib.CodecError, match="float64"):
        re.run(arenas0, [np.float64(v) for v in w], re.pack(base))
    assert re.optimizer_state()["step"] == 0
    host = [Restated(kind, p, **hyper) for p in params]
    first = None
    for rnd in range(2):    # the second round's base is the first's new model
        collabs = [[(b + rng.standard_normal(b.shape) * 0.02).astype(F) for b in base] for _ in range(C)]
        aggs = [host[i].step([c[i] for c in collabs], w, base[i]) for i in range(len(shapes))]
        np.random.seed(11 + rnd)
        ref_pay, ref_models = _reference_round(pipe, shapes, aggs, base)
        after_ref = np.random.randint(0, 2 ** 31)
        arenas, base_a = [re.pack(c) for c in collabs], re.pack(base)
        agg = torch.empty(re.arena_numel, dtype=torch.float32, device=DEV)
        np.random.seed(11 + rnd)
        new, pay, seeds = re.run(arenas, w, base_a, agg_out=agg)
        assert np.random.randint(0, 2 ** 31) == after_ref          # one draw per tensor, in order
        st = re.optimizer_state()
        assert st["step"] == rnd + 1 and (st["first_moment"] is None) == (kind == "adagrad")
        for i, s in enumerate(shapes):
            what = f"{kind} round {rnd} tensor {i}"
            assert_same_bits(re.view(agg, i).cpu().numpy(), aggs[i], what + " agg_out")
            assert pay[i][0] == ref_pay[i][0], what
            assert pay[i][1] == ref_pay[i][1], what
            np.testing.assert_array_equal(re.view(new, i).cpu().numpy(), ref_models[i], err_msg=what)
            assert_same_bits(re.view(st["params"], i).cpu().numpy(), host[i].p, what + " p")
            assert_same_bits(re.view(st["second_moment"], i).cpu().numpy(), host[i].v, what + " v")
            if kind != "adagrad":
                assert_same_bits(re.view(st["first_moment"], i).cpu().numpy(), host[i].m, what + " m")
        assert [seeds[i] for i in big] == _seeds_of(ref_pay, re.numels, re.dim_threshold)
        if first is None:
            first = (arenas, base_a, new, seeds)
        base = ref_models
    # a second instance repeats round 0 in place (out aliases the base arena), nothing downloaded
    arenas, base_a, new, seeds = first
    re2 = RoundEnd(pipe, shapes, DEV, aggregation=kind, optimizer=hyper)
    re2.init_optimizer(re2.pack(params))
    inplace = base_a.clone()
    np.random.seed(11)
    got, none, dev_seeds = re2.run(arenas, w, inplace, payloads=False, out=inplace)
    assert got is inplace and none is None and dev_seeds.is_cuda
    assert [int(v) for v in dev_seeds.cpu()] == seeds
    assert re2.optimizer_state()["step"] == 1
    for i in range(len(shapes)):
        assert torch.equal(re2.view(inplace, i), re2.view(new, i)), i


# --------------------------------------------- the existing aggregations, unchanged ---
@pytest.mark.parametrize("aggregation", ["weighted_average", "median"])
def test_round_end_existing_aggregations_unchanged(aggregation):
    from openfl_amd import _lib
    from openfl_amd.aggregation import AGGREGATIONS, RoundEnd
    from openfl_amd.pipelines import EdenPipeline
    assert AGGREGATIONS == ("weighted_average", "median", "geometric_median")
    rng = np.random.default_rng(2)
    shapes = [(64,), (1,), (70_000,), (5000,), (3, 5)]
    collabs = [[(rng.standard_normal(s) * 0.01).astype(F) for s in shapes] for _ in range(3)]
    base = [(rng.standard_normal(s) * 0.1).astype(F) for s in shapes]
    w = [0.2, 0.5, 0.3]
    pipe = EdenPipeline(n_bits=8, device=DEV, seed_mode="fast")
    if aggregation == "median":
        aggs = [np.median(np.array([c[i] for c in collabs]), axis=0) for i in range(len(shapes))]
    else:
        aggs = [np.average([c[i] for c in collabs], weights=w, axis=0) for i in range(len(shapes))]
    np.random.seed(3)
    ref_pay, ref_models = _reference_round(pipe, shapes, aggs, base)
    re = RoundEnd(pipe, shapes, DEV, aggregation=aggregation)
    assert re.fused == (aggregation == "weighted_average")
    np.random.seed(3)
    new, pay, seeds = re.run([re.pack(c) for c in collabs], w, re.pack(base))
    for i in range(len(shapes)):
        assert pay[i][0] == ref_pay[i][0] and pay[i][1] == ref_pay[i][1], i
        np.testing.assert_array_equal(re.view(new, i).cpu().numpy(), ref_models[i], err_msg=str(i))
    with pytest.raises(_lib.CodecError):
        re.init_optimizer(re.pack(base))
    with pytest.raises(_lib.CodecError):
        RoundEnd(pipe, shapes, DEV, aggregation=aggregation, optimizer={"learning_rate": 0.1})
    with pytest.raises(_lib.CodecError):
        RoundEnd(pipe, shapes, DEV, aggregation="trimmed_mean")
