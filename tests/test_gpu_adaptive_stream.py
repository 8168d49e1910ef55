"""GPU: the FedOpt optimisers one collaborator at a time -- the two kernels
against the NumPy float32 restatement and ofl_adaptive_step bit for bit,
RoundEnd.accumulator(base_arena=) / add / finish against run() over two rounds,
and the refusals, each raised before anything is launched or drawn."""
import gzip

import numpy as np
import pytest
import torch

from tests.round_stream_cases import DEV, F, SHAPES_ROW, bits, make_pipeline, md_key, rng_state, tensors
from tests.test_adaptive_aggregation_cpu import Restated, assert_same_bits
from tests.test_gpu_adaptive_aggregation import CUSTOM, KINDS

pytestmark = pytest.mark.gpu
# adam: the defaults; yogi's betas[1] >= 0.5 keeps its second moment >= 0, so no NaN reaches the seed formula
RE_HYPER = {"adam": {}, "yogi": dict(learning_rate=0.02, betas=(0.8, 0.95), initial_accumulator_value=0.01, epsilon=1e-6),
            "adagrad": dict(learning_rate=0.02, initial_accumulator_value=0.25, epsilon=1e-3)}


def _case(n, C, seed):
    """base, C collaborators, p, m, v of n float32 values; the last min(n, 5)
    columns are designed: base == x everywhere and p = -0.0 (a -0.0 first
    product under a negative weight: g must be +0.0, which p's sign shows);
    differences of 1.5e-38 (denormal products under weights below 1); an inf in
    the collaborator whose weight is 0 (NaN); 3e38 - -3e38 (inf); a NaN."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(n, dtype=F) * F(0.1)
    xs = [base + rng.standard_normal(n, dtype=F) * F(0.02) for _ in range(C)]
    p, m, v = (np.abs(rng.standard_normal(n, dtype=F)) * F(s) for s in (0.1, 0.01, 0.01))
    zero_c = min(1, C - 1)
    for k, col in enumerate(range(n - 1, max(n - 6, -1), -1)):
        for c, x in enumerate(xs):
            x[col] = base[col]
            if k == 1:
                base[col], x[col] = 0.0, F(-1.5e-38)
            if k == 2 and c == zero_c:
                x[col] = np.inf
            if k == 3 and c == 0:
                base[col], x[col] = F(3e38), F(-3e38)
            if k == 4 and c == 0:
                x[col] = np.nan
        if k == 0:
            p[col] = F(-0.0)
    return base, xs, p, m, v


def _weights(C):
    """A negative first weight and a zero one; one collaborator: each in turn."""
    rest = [float(w) for w in np.random.default_rng(C).random(max(C - 2, 0)) * 0.8 + 0.1]
    return [[-0.75], [0.0]] if C == 1 else [[-0.75, 0.0] + rest]


def _dev(a, offset):
    """As allocated, or the view one element into a larger tensor (the scalar path)."""
    big = torch.zeros(offset + a.size + 3, dtype=torch.float32, device=DEV)
    big[offset:offset + a.size] = torch.from_numpy(a).to(DEV)
    return big[offset:offset + a.size]


def _stream_against_restated(kind, C, n, offset, w, step_too):
    from openfl_amd import aggregation as A
    hyper = A.AdaptiveHyper(kind, **CUSTOM[kind])
    base, xs, p0, m0, v0 = _case(n, C, 1000 * C + n)
    r = Restated(kind, p0, **CUSTOM[kind])
    r.m, r.v = m0.copy(), v0.copy()
    with np.errstate(all="ignore"):
        g1 = F(0.0) + F(w[0]) * (base - xs[0])          # the chain's first link
    ref_p = r.step(xs, w, base)
    what = f"{kind} C={C} n={n} offset={offset} w0={w[0]}"
    b, dx = _dev(base, offset), [_dev(x, offset) for x in xs[:17]]      # more collaborators reuse 17 device buffers
    g = _dev(np.full(n, 7.0, F), offset)
    state = lambda: [None if a is None else _dev(a, offset) for a in (p0, None if kind == "adagrad" else m0, v0)]  # noqa: E731
    (p, m, v), agg, delta = state(), _dev(np.zeros(n, F), offset), _dev(np.zeros(n, F), offset)
    for c, x in enumerate(xs):
        d = dx[c % 17]
        if c >= 17:
            d.copy_(torch.from_numpy(x))
        A.adaptive_accumulate(d, F(w[c]), b, n, g, c == 0, device=DEV)
        if c == 0:
            assert_same_bits(g.cpu().numpy(), g1, what + " g after the first add")
    A.adaptive_finish(hyper, 0, g, b, n, p, m, v, agg_out=agg, delta_out=delta, device=DEV)
    with np.errstate(all="ignore"):
        want = {"p": ref_p, "v": r.v, "agg_out": ref_p, "delta_out": ref_p - base, **({} if m is None else {"m": r.m})}
    got = {"p": p, "m": m, "v": v, "agg_out": agg, "delta_out": delta}
    for k, ref in want.items():
        assert_same_bits(got[k].cpu().numpy(), ref, f"{what} {k}")
    if step_too:
        (p2, m2, v2), agg2, delta2 = state(), torch.zeros_like(agg), torch.zeros_like(delta)
        A.adaptive_step(hyper, 0, dx[:C], np.asarray(w, F), b, n, p2, m2, v2, agg_out=agg2, delta_out=delta2, device=DEV)
        for k, t in {"p": p2, "m": m2, "v": v2, "agg_out": agg2, "delta_out": delta2}.items():
            if t is not None:
                assert_same_bits(got[k].cpu().numpy(), t.cpu().numpy(), f"{what} {k} against ofl_adaptive_step")


@pytest.mark.parametrize("C", [1, 2, 17, 130])
@pytest.mark.parametrize("kind", KINDS)
def test_kernels_equal_numpy_and_the_step(kind, C):
    """n = 1, 7 (tail only), 4 * 256 + 3 (a quad per thread of a block and a
    tail), the same one element into a larger tensor (scalar), and 15 * 1024 + 3
    (two blocks: one takes 8 quads per lane at once, the other single quads)."""
    for n, offset in ((1, 0), (7, 0), (4 * 256 + 3, 0), (4 * 256 + 3, 1), (15 * 1024 + 3, 0)):
        for w in _weights(C):
            _stream_against_restated(kind, C, n, offset, w, step_too=C <= 17)


def test_kernels_second_loop_trip():
    """Beyond the capped grid (16 blocks per CU x 256 threads x 4 elements a
    trip): the accumulate's lanes take 8 quads per trip, so 15 trips and a half
    are a second 8-quad trip for half the lanes, single quads for the rest and
    a tail; the finish's one-quad loop takes 16 trips."""
    trip = torch.cuda.get_device_properties(0).multi_processor_count * 16 * 256 * 4
    _stream_against_restated("adagrad", 2, 15 * trip + trip // 2 + 7, 0, _weights(2)[0], step_too=False)


def _opt_bits(re):
    st = re.optimizer_state()
    return [st["step"]] + [None if t is None else bits(t.cpu().numpy()) for t in
                           (st["params"], st["first_moment"], st["second_moment"])]


@pytest.mark.parametrize("kind,name,upload", [("adam", "eden_fast", False), ("yogi", "eden_fast", True),
                                              ("adagrad", "eden_fast", False), ("adam", "kc", False)])
def test_streamed_round_equals_run(kind, name, upload):
    """Two consecutive rounds of 3 collaborators on a layout with 1-element
    tensors, tensors at and below dim_threshold and a row-pass slice; with
    upload the collaborators come as the pipeline's own payloads."""
    from openfl_amd.aggregation import RoundEnd
    pipe, shapes, w = make_pipeline(name), list(SHAPES_ROW), [0.5, 2.0, 1.25]
    res = [RoundEnd(pipe, shapes, device=DEV, aggregation=kind, optimizer=RE_HYPER[kind]) for _ in range(2)]
    for re in res:
        re.init_optimizer(re.pack(tensors(shapes, 3, 0.1)))
    base = [re.pack(tensors(shapes, 7, 0.1)) for re in res]
    for rnd in range(2):
        deltas = [tensors(shapes, 1000 + 10 * rnd + c) for c in range(3)]
        items = [[pipe.forward(d) for d in ds] for ds in deltas] if upload else None
        done = []
        for k, re in enumerate(res):
            if upload:
                xs = [re.ingest(it, base_arena=base[k]) for it in items] if k == 0 else items
            else:
                xs = [base[k] + re.pack(ds) for ds in deltas]
            np.random.seed(40 + rnd)
            if k == 0:
                new, pay, seeds = re.run(xs, w, base[k])
            else:
                acc = re.accumulator(base_arena=base[k])
                for x, wc in zip(xs, w):
                    acc.add_upload(x, wc, base_arena=base[k]) if upload else acc.add(x, wc)
                new, pay, seeds = re.finish(acc, base_arena=base[k])
            done.append((new.cpu().numpy(), pay, seeds, rng_state(), _opt_bits(re)))
            base[k] = new
        (m1, p1, *rest1), (m2, p2, *rest2) = done      # rest: seeds, np.random state, optimiser state
        assert bits(m2) == bits(m1) and rest2 == rest1 and rest1[2][0] == rnd + 1
        for i, ((pg, mg), (pw, mw)) in enumerate(zip(p2, p1)):
            if name == "kc" and re.numels[i] < 6:      # the host gzip's header carries a time stamp
                pg, pw = gzip.decompress(pg), gzip.decompress(pw)
            assert pg == pw and md_key(mg) == md_key(mw), i


def test_refusals_come_before_any_launch_or_draw():
    from openfl_amd._lib import CodecError
    from openfl_amd.aggregation import RoundEnd
    pipe, shapes = make_pipeline("eden_fast"), list(SHAPES_ROW)
    re, other = (RoundEnd(pipe, shapes, device=DEV, aggregation="adam") for _ in range(2))
    base, x = re.pack(tensors(shapes, 7, 0.1)), re.pack(tensors(shapes, 8, 0.1))
    np.random.seed(9)
    before = rng_state()
    with pytest.raises(CodecError, match="init_optimizer"):
        re.accumulator(base_arena=base)
    for r in (re, other):
        r.init_optimizer(base)
    state = _opt_bits(re)
    with pytest.raises(CodecError, match="base_arena is required"):
        re.accumulator()
    with pytest.raises(CodecError, match="float32"):
        re.accumulator(sums=torch.empty(re.arena_numel, dtype=torch.float64, device=DEV), base_arena=base)
    acc = re.accumulator(base_arena=base)
    acc.sums.fill_(5.0)
    with pytest.raises(CodecError, match="float64"):
        acc.add(x, np.float64(1.0))
    assert acc.weights == [] and bool((acc.sums == 5.0).all())
    acc.add(x, 1.0)
    with pytest.raises(CodecError, match="the accumulator was made with"):
        re.finish(acc, base_arena=x)
    with pytest.raises(CodecError, match="of this RoundEnd"):
        other.finish(acc)
    assert rng_state() == before and not acc.finished and _opt_bits(re) == state and _opt_bits(other) == state
    re.finish(acc, base_arena=base, payloads=False)
    after, state = rng_state(), _opt_bits(re)
    assert after != before and state[0] == 1
    with pytest.raises(CodecError, match="after finish"):
        re.finish(acc)
    with pytest.raises(CodecError, match="after finish"):
        acc.add(x, 1.0)
    assert rng_state() == after and _opt_bits(re) == state
