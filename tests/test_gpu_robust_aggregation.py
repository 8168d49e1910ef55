"""GPU: the robust aggregators (csrc/agg_kernels.hip: ofl_median_delta,
ofl_gmedian_delta, ofl_agg_delta_seeds) and RoundEnd(aggregation=...).

Median is compared with np.median by value (median.py:48-49).  Geometric
median is compared with the reference's own results (tests/golden/
geometric_median_golden.*, geometric_median.py:27-56) within
    max|got - ref| <= 1e-10 * max|x|
(everything is float64; the only licensed difference is the order of the
distance sums, n u ~ 2^17 * 1.1e-16 ~ 1.5e-11 per distance through at most
five passes; a float32 accumulator (>= 1e-7) or a skipped or extra round
(>= 1e-4 on the outlier cases) is far outside).  RoundEnd with either
aggregator is compared bit for bit with the reference's per-tensor sequence
(aggregate -> generate_delta -> compress -> decompress -> apply_delta) run
with the same pipeline through the host API."""
import warnings

import numpy as np
import pytest
import torch

from tests import agg_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GM_RTOL = 1e-10


# ------------------------------------------------------------------ median ---
MEDIAN_SHAPES = [(), (1,), (2,), (3,), (5,), (7, 13), (1027,), (3, 1, 5), (4099,)]


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 8, 15, 16, 17, 33])
def test_median_equals_numpy(C):
    """The 16-byte body, the scalar tail, the register path (C <= 16) and the
    LDS path (C > 16); the plugin through LocalTensor."""
    from openfl_amd.aggregation import Median, median
    from openfl_amd.tensor_codec import LocalTensor
    for shape in MEDIAN_SHAPES:
        rng = np.random.default_rng(C * 100 + len(shape) + 7 * int(np.prod(shape)))
        xs = [np.asarray(rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 3)).astype(np.float32)
              for _ in range(C)]
        ref = np.median(np.array(xs), axis=0)
        got = median(xs, DEV)
        assert got.dtype == np.float32 and got.shape == ref.shape, shape
        np.testing.assert_array_equal(got, ref, err_msg=str(shape))
        lt = [LocalTensor(f"c{i}", x, float(i)) for i, x in enumerate(xs)]  # the weights are ignored
        np.testing.assert_array_equal(Median(DEV).call(lt), ref, err_msg=str(shape))
        np.testing.assert_array_equal(Median(DEV)(lt, None, "t", 0, ()), ref, err_msg=str(shape))


@pytest.mark.parametrize("C", [4, 5])
def test_median_designed_columns(C):
    """Duplicates, all-equal columns, +-inf, 3e38 pairs whose float32 sum
    overflows, a NaN in every row position, +-0.0 ties -- NaN exactly where
    NumPy puts it (assert_array_equal treats NaNs as equal, and -0.0 == 0.0)."""
    from openfl_amd.aggregation import median
    inf, nan = np.inf, np.nan
    cols = [[1, 1, 2, 2, 3], [2, 1, 2, 1, 2], [7, 7, 7, 7, 7], [-1, -1, -1, 5, 5],
            [inf, 1, 2, -inf, 3], [inf, inf, 1, 2, inf], [-inf, inf, inf, -inf, 0], [-inf, -inf, -inf, -inf, -inf],
            [inf, inf, inf, inf, inf], [-inf, -inf, inf, inf, 1],
            [3e38, 3e38, 1, 3.2e38, 3.1e38], [-3e38, -3e38, -3.3e38, 0, -3.2e38], [3e38, 3e38, 3e38, 3e38, 3e38],
            [0.0, -0.0, 0.0, -0.0, 0.0], [-0.0, -0.0, 0.0, 0.0, -0.0], [-1, 0.0, -0.0, 1, -0.0],
            [1e-45, 3e-45, 1e-45, 3e-45, 1e-45]]
    for r in range(C):  # a NaN in each row position, with and without infinities beside it
        c = [float(k) for k in range(5)]
        c[r] = nan
        cols.append(c)
        c = [inf, -inf, inf, -inf, inf]
        c[r] = nan
        cols.append(c)
    cols.append([nan] * 5)
    stack = np.asarray(cols, np.float32).T[:C]           # (C, columns)
    stack = np.concatenate([stack, stack[:, ::-1]], axis=1)  # 2 x 28 columns: body and tail
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        ref = np.median(stack, axis=0)
    assert np.isnan(ref).sum() >= 2 * (2 * C + 1) and np.isinf(ref).any()
    got = median(list(stack), DEV)
    np.testing.assert_array_equal(got, ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref))


def test_median_errors():
    from openfl_amd import _lib
    from openfl_amd.aggregation import median
    x = np.ones(4, np.float32)
    with pytest.raises(_lib.CodecError):
        median([x, x.astype(np.float64)], DEV)
    with pytest.raises(_lib.CodecError):
        median([x, np.ones(5, np.float32)], DEV)
    with pytest.raises(_lib.CodecError):
        median([], DEV)
    with pytest.raises(_lib.CodecError, match="128"):
        median([x] * 129, DEV)
    # the limit is the library's own, too
    t = torch.ones(8, dtype=torch.float32, device=DEV)
    ptrs = np.asarray([t.data_ptr()] * 129, np.uint64)
    rc = _lib.lib().ofl_median_delta(129, ptrs.ctypes.data, None, 8, t.data_ptr(), None,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.OFL_EINVAL and b"128" in _lib.lib().ofl_agg_last_error()
    np.testing.assert_array_equal(median([x] * 128, DEV), x)


# -------------------------------------------------------- geometric median ---
@pytest.fixture(scope="module")
def golden():
    return agg_golden.load()


def _gm_tol(xs):
    return GM_RTOL * max(float(np.abs(x).max()) for x in xs)


@pytest.mark.parametrize("name", ["c5_shift", "c3_small_scale", "c3_chunks", "c16_outlier", "c2_equal_513",
                                  "c2_equal_1", "c1_single", "c3_identical"])
def test_geometric_median_matches_reference(golden, name):
    from openfl_amd.aggregation import GeometricMedian, geometric_median
    from openfl_amd.tensor_codec import LocalTensor
    arrays, index = golden
    case = next(c for c in index["cases"] if c["name"] == name)
    xs, w, ref = agg_golden.inputs(arrays, name), arrays["w_" + name], arrays["ref_" + name]
    got, rounds = geometric_median(xs, w, device=DEV, return_iterations=True)
    assert got.dtype == np.float64 and got.shape == ref.shape
    err = float(np.abs(got - ref).max())
    print(f"{name}: max|got - ref| = {err:.3e}, bound {_gm_tol(xs):.3e}, rounds {rounds} (reference {case['rounds']})")
    assert err <= _gm_tol(xs)
    if case["assert_rounds"]:
        assert rounds == case["rounds"]
    again = geometric_median(xs, w, device=DEV)
    assert again.tobytes() == got.tobytes()      # no atomics: the same bits on every run
    lt = [LocalTensor(f"c{i}", x, wi) for i, (x, wi) in enumerate(zip(xs, w))]
    assert GeometricMedian(DEV).call(lt).tobytes() == got.tobytes()


def test_geometric_median_many_chunks():
    """n = 2^17 + 5, two collaborators with equal weights: 33 chunks per
    tensor through the two-stage reduction; the weights stay equal, so the
    result is the plain average and the reference's test stops after round 1."""
    from openfl_amd.aggregation import geometric_median
    rng = np.random.default_rng(5)
    xs = [rng.standard_normal((1 << 17) + 5).astype(np.float32) for _ in range(2)]
    got, rounds = geometric_median(xs, [1.0, 1.0], device=DEV, return_iterations=True)
    ref = np.average(xs, weights=[1.0, 1.0], axis=0)
    err = float(np.abs(got - ref).max())
    print(f"many chunks: max|got - ref| = {err:.3e}, bound {_gm_tol(xs):.3e}, rounds {rounds}")
    assert err <= _gm_tol(xs)
    assert rounds == 1


def test_geometric_median_parameters_and_errors():
    from openfl_amd import _lib
    from openfl_amd.aggregation import geometric_median
    rng = np.random.default_rng(9)
    xs = [rng.standard_normal(700).astype(np.float32) for _ in range(3)]
    xs[1] = xs[1] + np.float32(4)
    w = [1.0, 1.0, 1.0]
    avg, r0 = geometric_median(xs, w, maxiter=0, device=DEV, return_iterations=True)
    assert r0 == 0
    np.testing.assert_allclose(avg, np.average(xs, weights=w, axis=0), rtol=0, atol=_gm_tol(xs))
    one, r1 = geometric_median(xs, w, maxiter=1, device=DEV, return_iterations=True)
    assert r1 == 1 and np.abs(one - avg).max() > 1e-3           # the outlier is down-weighted
    loose, rl = geometric_median(xs, w, ftol=1e9, device=DEV, return_iterations=True)
    assert rl == 1 and loose.tobytes() == one.tobytes()         # the test stops it after the first round
    with pytest.raises(_lib.CodecError, match="16"):
        geometric_median([xs[0]] * 17, [1.0] * 17, device=DEV)
    with pytest.raises(ZeroDivisionError):
        geometric_median(xs, [0.0, 0.0, 0.0], device=DEV)
    with pytest.raises(_lib.CodecError):
        geometric_median([xs[0], xs[1].astype(np.float64)], [1.0, 1.0], device=DEV)
    with pytest.raises(_lib.CodecError):
        geometric_median([xs[0], xs[1][:5]], [1.0, 1.0], device=DEV)
    with pytest.raises(_lib.CodecError):
        geometric_median([], [], device=DEV)


# ---------------------------------------------------------------- RoundEnd ---
SHAPES = [(64, 3, 3, 3), (64,), (1,), (300, 200), (5000,), (2, 2), (1 << 18,), (100,), (101,), (60001,), (3, 20001)]


def _reference_round(pipe, shapes, aggs, base):
    """_prepare_trained per tensor with the host API, from the aggregate on:
    generate_delta -> compress -> decompress -> apply_delta."""
    from openfl_amd.tensor_codec import TensorCodec, TensorKey
    tc = TensorCodec(pipe)
    payloads, models = [], []
    for i, s in enumerate(shapes):
        key = TensorKey(f"t{i}", "aggregator_x", 0, False, ("aggregated",))
        if base is not None:
            dk, delta = tc.generate_delta(key, aggs[i], base[i])
        else:
            dk, delta = key, aggs[i]
        ck, payload, md = tc.compress(dk, delta)
        payloads.append((payload, [dict(m) for m in md]))
        _, dec = tc.decompress(ck, payload, md)
        if base is not None:
            _, new = tc.apply_delta(dk, dec, base[i])
        else:
            new = dec
        models.append(np.asarray(new, np.float32))
    return payloads, models


def _seeds_of(payloads, numels, threshold):
    return [int(md[0]["int_to_float"][0]) for (_, md), n in zip(payloads, numels) if n > threshold]


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("with_base", [True, False])
@pytest.mark.parametrize("seed_mode", ["fast", "reference"])
def test_round_end_median_matches_per_tensor(seed_mode, with_base, C):
    from openfl_amd import _lib
    from openfl_amd.aggregation import RoundEnd
    from openfl_amd.pipelines import EdenPipeline
    rng = np.random.default_rng(70 + C)
    collabs = [[(rng.standard_normal(s) * 0.01).astype(np.float32) for s in SHAPES] for _ in range(C)]
    base = [(rng.standard_normal(s) * 0.1).astype(np.float32) for s in SHAPES] if with_base else None
    pipe = EdenPipeline(n_bits=8, device=DEV, seed_mode=seed_mode)
    aggs = [np.median(np.array([c[i] for c in collabs]), axis=0) for i in range(len(SHAPES))]
    assert all(a.dtype == np.float32 for a in aggs)
    np.random.seed(11)
    ref_pay, ref_models = _reference_round(pipe, SHAPES, aggs, base)
    after_ref = np.random.randint(0, 2 ** 31)

    re = RoundEnd(pipe, SHAPES, DEV, aggregation="median")
    assert not re.fused
    arenas = [re.pack(c) for c in collabs]
    base_a = re.pack(base) if with_base else None
    agg = torch.empty(re.arena_numel, dtype=torch.float32, device=DEV)
    np.random.seed(11)
    new, pay, seeds = re.run(arenas, None, base_a, agg_out=agg)
    assert np.random.randint(0, 2 ** 31) == after_ref          # one draw per tensor, in order
    for i, s in enumerate(SHAPES):
        assert re.view(agg, i).cpu().numpy().tobytes() == aggs[i].tobytes(), i
        assert pay[i][0] == ref_pay[i][0], i
        assert pay[i][1] == ref_pay[i][1], i
        np.testing.assert_array_equal(re.view(new, i).cpu().numpy(), ref_models[i].reshape(s), err_msg=str(i))
    big = [i for i, n in enumerate(re.numels) if n > re.dim_threshold]
    assert [seeds[i] for i in big] == _seeds_of(ref_pay, re.numels, re.dim_threshold)
    with pytest.raises(_lib.CodecError):  # agg_out of the weighted average's dtype is refused
        re.run(arenas, None, base_a, agg_out=agg.double())
    np.random.seed(11)
    if with_base:  # in-place model update (out aliases the base arena), nothing downloaded
        inplace = base_a.clone()
        _, none, dev_seeds = re.run(arenas, None, inplace, payloads=False, out=inplace)
        assert none is None and dev_seeds.is_cuda
        assert [int(v) for v in dev_seeds.cpu()] == seeds
        for i in range(len(SHAPES)):
            assert torch.equal(re.view(inplace, i), re.view(new, i)), i


@pytest.mark.parametrize("seed_mode", ["fast", "reference"])
def test_round_end_geometric_median_matches_per_tensor(seed_mode):
    from openfl_amd.aggregation import RoundEnd, geometric_median
    from openfl_amd.pipelines import EdenPipeline
    rng = np.random.default_rng(33)
    shapes = [(64, 3, 3, 3), (64,), (1,), (300, 200), (5000,), (2, 2), (70_001,), (100,), (101,)]
    C = 3
    collabs = [[(rng.standard_normal(s) * 0.01).astype(np.float32) for s in shapes] for _ in range(C)]
    collabs[2] = [x * np.float32(25) + np.float32(0.3) for x in collabs[2]]  # the outlier collaborator
    base = [(rng.standard_normal(s) * 0.1).astype(np.float32) for s in shapes]
    w = [0.2, 0.5, 0.3]
    pipe = EdenPipeline(n_bits=8, device=DEV, seed_mode=seed_mode)
    re = RoundEnd(pipe, shapes, DEV, aggregation="geometric_median")
    assert not re.fused
    arenas = [re.pack(c) for c in collabs]
    base_a = re.pack(base)
    agg = torch.zeros(re.arena_numel, dtype=torch.float64, device=DEV)
    np.random.seed(19)
    new, pay, seeds = re.run(arenas, w, base_a, agg_out=agg)
    after = np.random.randint(0, 2 ** 31)
    aggs = [re.view(agg, i).cpu().numpy() for i in range(len(shapes))]
    for i, s in enumerate(shapes):
        xs = [c[i] for c in collabs]
        alone = geometric_median(xs, w, device=DEV)
        assert np.abs(aggs[i] - alone).max() <= _gm_tol(xs), i
        assert aggs[i].tobytes() == alone.tobytes(), i          # the same chunks, the same order
        plain = np.average(xs, weights=w, axis=0)
        assert np.abs(aggs[i] - plain).max() > 1e-4, i          # not the weighted average
    # the codec side, exactly: the host sequence fed the aggregate the device produced
    np.random.seed(19)
    ref_pay, ref_models = _reference_round(pipe, shapes, aggs, base)
    assert np.random.randint(0, 2 ** 31) == after
    for i, s in enumerate(shapes):
        assert pay[i][0] == ref_pay[i][0], i
        assert pay[i][1] == ref_pay[i][1], i
        np.testing.assert_array_equal(re.view(new, i).cpu().numpy(), ref_models[i].reshape(s), err_msg=str(i))
    big = [i for i, n in enumerate(re.numels) if n > re.dim_threshold]
    assert [seeds[i] for i in big] == _seeds_of(ref_pay, re.numels, re.dim_threshold)
    # without agg_out and without payloads: the same model, nothing downloaded
    np.random.seed(19)
    new2, none, dev_seeds = re.run(arenas, w, base_a, payloads=False)
    assert none is None and [int(v) for v in dev_seeds.cpu()] == seeds
    assert torch.equal(new2, new)
    with pytest.raises(ZeroDivisionError):
        re.run(arenas, [0.0, 0.0, 0.0], base_a)


def test_round_end_default_aggregation_unchanged():
    from openfl_amd import _lib
    from openfl_amd.aggregation import RoundEnd
    from openfl_amd.pipelines import EdenPipeline
    rng = np.random.default_rng(2)
    shapes = [(64,), (1,), (70_000,), (5000,)]
    collabs = [[(rng.standard_normal(s) * 0.01).astype(np.float32) for s in shapes] for _ in range(3)]
    base = [(rng.standard_normal(s) * 0.1).astype(np.float32) for s in shapes]
    w = [0.2, 0.5, 0.3]
    pipe = EdenPipeline(n_bits=8, device=DEV, seed_mode="fast")
    outs = []
    for kw in ({}, {"aggregation": "weighted_average"}):
        re = RoundEnd(pipe, shapes, DEV, **kw)
        assert re.fused and re.aggregation == "weighted_average"
        np.random.seed(3)
        outs.append(re.run([re.pack(c) for c in collabs], w, re.pack(base)))
    assert outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]
    assert torch.equal(outs[0][0], outs[1][0])
    with pytest.raises(_lib.CodecError):
        RoundEnd(pipe, shapes, DEV, aggregation="trimmed_mean")
    with pytest.raises(_lib.CodecError, match="16"):
        re = RoundEnd(pipe, shapes, DEV, aggregation="geometric_median")
        re.run([re.pack(collabs[0])] * 17, [1.0] * 17, re.pack(base))
