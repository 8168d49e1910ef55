"""The aggregator's end-of-round tensor work on the device.

Reference (paths relative to /root/reference/openfl):
  interface/aggregation_functions/weighted_average.py:12-58
      WeightedAverage.call -> np.average(tensors, weights=weights, axis=0)
  component/aggregator/aggregator.py:780-865  _prepare_trained, per tensor:
      agg = WeightedAverage(local tensors)            (float64)
      delta = TensorCodec.generate_delta(agg, base)   (agg - base, float64)
      payload, md = TensorCodec.compress(delta)       (the compression pipeline)
      dec = TensorCodec.decompress(payload, md)       (float32)
      model = TensorCodec.apply_delta(dec, base)      (base + dec, float32)
  pipelines/tensor_codec.py:150-211  generate_delta / apply_delta

RoundEnd does that for every tensor of a model update in one device pass
sequence over flat arenas (csrc/agg_kernels.hip + the Eden plan): average +
delta in one kernel (float64 arithmetic in NumPy's order, delta rounded to
float32 as Eden.compress does), the seeds' serial sums from the delta's values
summed on the device (fast mode: a 4096-element prefix per tensor, reference
mode: all of it, one lane per tensor in Python's left-to-right order) and
hashed there with CPython's float hash (no host round trip), one
Eden encode and decode of all the big tensors, and apply_delta in place.  The
payloads, metadata, np.random draws and new model are identical to calling
the reference's functions tensor by tensor with an openfl_amd EdenPipeline
(tests/test_gpu_aggregation.py).  No CPU fallback: without the library or a
GPU every call raises CodecError.

RoundEnd takes a KCPipeline, SKCPipeline or STCPipeline too: the same
aggregation kernels, then _LossyTail instead of the Eden seeds, encode and
decode (batched k-means with one np.random seed per tensor, one labelling +
decode + apply pass; DESIGN.md 3.9, tests/test_gpu_lossy_round_end.py).

RoundEnd.ingest takes one collaborator's upload (payload bytes + metadata per
tensor, as the aggregator receives them) to a device arena, and
RoundEnd.accumulator / finish take the weighted average one collaborator at
a time (ofl_wavg_accumulate, ofl_wavg_finish) with run()'s results bit for
bit (tests/test_gpu_round_ingest.py, test_gpu_round_stream.py).

Beside the weighted average: Median and GeometricMedian, and the FedOpt
server optimisers AdamAdaptiveAggregation, YogiAdaptiveAggregation and
AdagradAdaptiveAggregation (core/adaptive_aggregation.py on
utilities/optimizers/numpy/*_optimizer.py), whose parameters and moments stay
on the device between rounds (ofl_adaptive_step).
"""
import collections
import ctypes
import zlib

import numpy as np
import torch

from openfl_amd import _lib, hostmem, lossy
from openfl_amd.codec import EdenPlan, resolve_device, slice_plan
from openfl_amd.pipelines.eden_pipeline import _FAST_SEED_PREFIX, _copy_many
from openfl_amd.pipelines.kc_pipeline import KCPipeline
from openfl_amd.pipelines.skc_pipeline import SKCPipeline
from openfl_amd.pipelines.stc_pipeline import STCPipeline, _topk_count, ternary_map

_ALIGN = 64
_ROW_TILE = 1 << 15  # slices above this go through the row passes (kRowLog)


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t):
    """A device tensor's address, None (NULL) for an absent one."""
    return t.data_ptr() if t is not None else None


def _ptrs(xs):
    """The host pointer table of device tensors; keep it alive across the call."""
    return np.asarray([x.data_ptr() for x in xs], np.uint64)


def _flat_to(arrs, device):
    return [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(device) for a in arrs]


def _f64_weights(weights, n):
    w = np.asarray(weights)
    if w.ndim != 1 or w.size != n:
        raise _lib.CodecError("one weight per collaborator tensor")
    if np.result_type(np.float32, w.dtype) != np.float64:
        raise _lib.CodecError("weights must promote float32 tensors to float64 (np.average result dtype)")
    return np.ascontiguousarray(w, np.float64)


def weight_sum(weights, ndim):
    """np.average's denominator for tensors of `ndim` dimensions: NumPy's own
    float64 sum of the broadcast weights (weighted_average.py:14)."""
    w = np.asarray(weights)
    stack = np.zeros((w.size,) + (1,) * ndim, np.float32)
    scl = np.average(stack, weights=w, axis=0, returned=True)[1]
    return float(np.asarray(scl).reshape(-1)[0])


def _f32_stack(name, tensors):
    arrs = [np.asarray(t) for t in tensors]
    if not arrs:
        raise _lib.CodecError(f"{name}: no tensors")
    shape = arrs[0].shape
    if any(a.shape != shape or a.dtype != np.float32 for a in arrs):
        raise _lib.CodecError(f"{name}: float32 tensors of one shape")
    return arrs, shape, int(np.prod(shape, dtype=np.int64))


def _check_collaborators(name, n, limit):
    if n > limit:
        raise _lib.CodecError(f"{name}: {n} collaborators, at most {limit} are supported")


class _Plugin:
    """What the AggregationFunction plugins share: __call__ -> call(local_tensors,
    ...) and, for the stateless ones, a constructor that takes the device."""

    def __init__(self, device=None):
        self.device = device

    def __call__(self, local_tensors, *args):
        return self.call(local_tensors, *args)


def _wavg_launch(xs, w64, wsum, base, n, agg=None, delta64=None, delta32=None, device=None):
    ptrs = _ptrs(xs)
    _lib.check_agg(_lib.lib().ofl_wavg_delta(
        len(xs), ptrs.ctypes.data, w64.ctypes.data, wsum, _ptr(base), int(n), _ptr(agg), _ptr(delta64), _ptr(delta32),
        _stream(device)))


def _points_launch(xs, w64, wsum, base, idx, agg, delta32, device, ws):
    ptrs = _ptrs(xs)
    ix = np.ascontiguousarray(idx, np.int64)
    L = _lib.lib()
    need = int(L.ofl_wavg_points_workspace_bytes(len(xs), ix.size))
    buf = ws(need)
    _lib.check_agg(L.ofl_wavg_delta_points(
        len(xs), ptrs.ctypes.data, w64.ctypes.data, wsum, _ptr(base), ix.size, ix.ctypes.data, _ptr(agg), None,
        _ptr(delta32), buf.data_ptr(), buf.numel(), _stream(device)))


class _Scratch:
    def __init__(self, device):
        self.device = device
        self.buf = None

    def __call__(self, nbytes):
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
        return self.buf


def weighted_average(tensors, weights, device=None):
    """np.average(tensors, weights=weights, axis=0) on the GPU
    (weighted_average.py:12-14): float32 tensors, float64 result, bit-exact."""
    dev = resolve_device(device)
    arrs, shape, n = _f32_stack("weighted_average", tensors)
    w64 = _f64_weights(weights, len(arrs))
    wsum = weight_sum(w64, len(shape))
    if wsum == 0.0:
        raise ZeroDivisionError("Weights sum to zero, can't be normalized")
    with torch.cuda.device(dev):
        xs = _flat_to(arrs, dev)
        agg = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        if n == 1:
            _points_launch(xs, w64, wsum, None, [0], agg, None, dev, _Scratch(dev))
        elif n:
            _wavg_launch(xs, w64, wsum, None, n, agg=agg, device=dev)
        return agg[:n].cpu().numpy().reshape(shape)


class WeightedAverage(_Plugin):
    """AggregationFunction plugin (weighted_average.py:17-58): call(local_tensors, ...)
    -> np.average of the LocalTensor tensors by their weights, on the GPU."""

    def call(self, local_tensors, *_):
        tensors, weights = zip(*[(x.tensor, x.weight) for x in local_tensors])
        return weighted_average(tensors, weights, self.device)


_MEDIAN_MAX_C = 128   # ofl_median_delta: <= 16 in registers, <= 128 through LDS
_GMEDIAN_MAX_C = 16   # ofl_gmedian_delta: one launch's collaborators, no chaining
_GM_CHUNK = 4096
_GM_CHUNK_DT = np.dtype([("start", "<i8"), ("len", "<i4"), ("tensor", "<i4")])  # ofl_gm_chunk
AGGREGATIONS = ("weighted_average", "median", "geometric_median")


def _median_launch(xs, base, n, med=None, delta=None, device=None):
    _check_collaborators("median", len(xs), _MEDIAN_MAX_C)
    ptrs = _ptrs(xs)
    _lib.check_agg(_lib.lib().ofl_median_delta(
        len(xs), ptrs.ctypes.data, _ptr(base), int(n), _ptr(med), _ptr(delta), _stream(device)))


def median(tensors, device=None):
    """np.median(tensors, axis=0) on the GPU (median.py:48-49): float32
    tensors, float32 result, equal by value (tied zeros may differ in sign);
    at most 128 tensors."""
    dev = resolve_device(device)
    arrs, shape, n = _f32_stack("median", tensors)
    _check_collaborators("median", len(arrs), _MEDIAN_MAX_C)
    with torch.cuda.device(dev):
        out = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        if n:
            _median_launch(_flat_to(arrs, dev), None, n, med=out, device=dev)
        return out[:n].cpu().numpy().reshape(shape)


class Median(_Plugin):
    """AggregationFunction plugin (median.py:12-49): call(local_tensors, ...) ->
    np.median of the LocalTensor tensors on the GPU; the weights are ignored,
    as in the reference."""

    def call(self, local_tensors, *_):
        return median([x.tensor for x in local_tensors], self.device)


def _gm_start_weights(weights, n):
    """geometric_median.py:41: np.asarray(weights) / sum(weights)."""
    _f64_weights(weights, n)
    w = np.asarray(weights)
    tot = sum(w)
    if tot == 0:
        raise ZeroDivisionError("Weights sum to zero, can't be normalized")
    return np.ascontiguousarray(w / tot, np.float64)


def _gm_chunk_table(offsets, numels):
    """ofl_gmedian_delta's chunk table: every tensor tiled in order by chunks of
    <= 4096 elements -> (records, first chunk of every tensor [T + 1])."""
    parts, first = [], [0]
    for t, (o, n) in enumerate(zip(offsets, numels)):
        k = (n + _GM_CHUNK - 1) // _GM_CHUNK
        at = _GM_CHUNK * np.arange(k, dtype=np.int64)
        c = np.zeros(k, _GM_CHUNK_DT)
        c["start"] = o + at
        c["len"] = np.minimum(_GM_CHUNK, n - at)
        c["tensor"] = t
        parts.append(c)
        first.append(first[-1] + k)
    return np.concatenate(parts) if parts else np.zeros(0, _GM_CHUNK_DT), np.asarray(first, np.int32)


class _GmLayout:
    """Device tables and workspace of ofl_gmedian_delta for one arena layout."""

    def __init__(self, offsets, numels, device):
        chunks, first = _gm_chunk_table(offsets, numels)
        self.ntensors = len(numels)
        self.nchunks = int(chunks.size)
        raw = np.frombuffer(chunks.tobytes() or bytes(_GM_CHUNK_DT.itemsize), np.uint8).copy()
        self.chunks = torch.from_numpy(raw).to(device)
        self.first = torch.from_numpy(first).to(device)
        self.iters = torch.zeros(max(self.ntensors, 1), dtype=torch.int32, device=device)
        need = int(_lib.lib().ofl_gmedian_workspace_bytes(self.ntensors, self.nchunks))
        self.ws = torch.empty(need, dtype=torch.uint8, device=device)

    def launch(self, xs, w0, maxiter, eps, ftol, base, agg=None, delta64=None, delta32=None, device=None):
        _check_collaborators("geometric_median", len(xs), _GMEDIAN_MAX_C)
        ptrs = _ptrs(xs)
        _lib.check_agg(_lib.lib().ofl_gmedian_delta(
            len(xs), ptrs.ctypes.data, w0.ctypes.data, int(maxiter), float(eps), float(ftol), _ptr(base), self.ntensors,
            self.chunks.data_ptr(), self.nchunks, self.first.data_ptr(), _ptr(agg), _ptr(delta64), _ptr(delta32),
            self.iters.data_ptr(), self.ws.data_ptr(), self.ws.numel(), _stream(device)))


def geometric_median(tensors, weights, maxiter=4, eps=1e-5, ftol=1e-6, device=None, return_iterations=False):
    """geometric_median(tensors, weights, maxiter, eps, ftol) of
    geometric_median.py:27-56 on the GPU: Weiszfeld's algorithm in float64 with
    the reference's sequence of passes and its break test.  float32 tensors
    (at most 16), float64 result; the distance sums run in another order than
    NumPy's, so the result agrees to summation rounding.  return_iterations:
    also the number of Weiszfeld rounds run."""
    dev = resolve_device(device)
    arrs, shape, n = _f32_stack("geometric_median", tensors)
    _check_collaborators("geometric_median", len(arrs), _GMEDIAN_MAX_C)
    w0 = _gm_start_weights(weights, len(arrs))
    with torch.cuda.device(dev):
        lay = _GmLayout([0], [n], dev)
        xs = _flat_to(arrs, dev) if n else [torch.zeros(1, dtype=torch.float32, device=dev) for _ in arrs]
        agg = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        lay.launch(xs, w0, maxiter, eps, ftol, None, agg=agg, device=dev)
        res = agg[:n].cpu().numpy().reshape(shape)
        return (res, int(lay.iters[0].item())) if return_iterations else res


class GeometricMedian(_Plugin):
    """AggregationFunction plugin (geometric_median.py:76-112): call(local_tensors,
    ...) -> geometric_median of the LocalTensor tensors by their weights, on the
    GPU (the reference's defaults: maxiter 4, eps 1e-5, ftol 1e-6)."""

    def call(self, local_tensors, *_):
        tensors, weights = zip(*[(x.tensor, x.weight) for x in local_tensors])
        return geometric_median(tensors, np.array(weights), device=self.device)


# ---- FedOpt server optimisers (core/adaptive_aggregation.py:38-113 on
# utilities/optimizers/numpy/{adam,yogi,adagrad}_optimizer.py) ------------------
ADAPTIVE_AGGREGATIONS = ("adam", "yogi", "adagrad")   # RoundEnd(aggregation=...) beside AGGREGATIONS
_ADAPTIVE_KIND = {"adam": 0, "yogi": 1, "adagrad": 2}  # OFL_ADAPTIVE_*
_ADAPTIVE_MAX_C = 128                                  # ofl_adaptive_step: <= 16 unrolled, <= 128 from a table


class _AdaptiveConsts(ctypes.Structure):  # ofl_adaptive_consts
    _fields_ = [("kind", ctypes.c_int32), ("lr", ctypes.c_float), ("beta1", ctypes.c_float),
                ("one_minus_beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("one_minus_beta2", ctypes.c_float),
                ("bias1", ctypes.c_float), ("bias2", ctypes.c_float), ("eps", ctypes.c_float)]


class AdaptiveHyper:
    """The hyper-parameters of one optimiser kind ("adam", "yogi", "adagrad"),
    checked as the reference checks them (adam_optimizer.py:75-87,
    adagrad_optimizer.py:68-76; the same ValueErrors) and with its defaults.
    They are Python floats, as a plan gives them."""

    def __init__(self, kind, learning_rate=0.01, betas=None, initial_accumulator_value=None, epsilon=None):
        if kind not in _ADAPTIVE_KIND:
            raise _lib.CodecError(f"optimiser kind must be one of {ADAPTIVE_AGGREGATIONS}, not {kind!r}")
        adagrad = kind == "adagrad"
        if adagrad and betas is not None:
            raise TypeError("adagrad has no betas")
        betas = (0.9, 0.999) if betas is None else betas
        if initial_accumulator_value is None:
            initial_accumulator_value = 0.1 if adagrad else 0.0
        if epsilon is None:
            epsilon = 1e-10 if adagrad else 1e-8
        if learning_rate < 0:
            raise ValueError(f"Invalid learning rate: {learning_rate}. Learning rate must be >= 0.")
        if not adagrad:
            if not 0.0 <= betas[0] < 1:
                raise ValueError(f"Invalid betas[0] value: {betas[0]}. betas[0] must be in [0, 1).")
            if not 0.0 <= betas[1] < 1:
                raise ValueError(f"Invalid betas[1] value: {betas[1]}. betas[1] must be in [0, 1).")
        if initial_accumulator_value < 0:
            raise ValueError(f"Invalid initial_accumulator_value value: {initial_accumulator_value}. "
                             "Initial accumulator value must be >= 0.")
        if epsilon <= 0:
            raise ValueError(f"Invalid epsilon value: {epsilon}. Epsilon avalue must be > 0.")
        self.kind = kind
        self.learning_rate = float(learning_rate)
        self.beta_1, self.beta_2 = float(betas[0]), float(betas[1])
        self.initial_accumulator_value = float(initial_accumulator_value)
        self.epsilon = float(epsilon)

    def consts(self, steps_taken):
        """ofl_adaptive_consts for the step after `steps_taken`: every Python-float
        expression of the reference evaluated in double, then rounded to
        float32 once (what NumPy does with a Python float beside a float32 array)."""
        f = lambda x: float(np.float32(x))  # noqa: E731
        b1, b2, t = self.beta_1, self.beta_2, int(steps_taken) + 1
        if self.kind == "adagrad":
            return _AdaptiveConsts(2, f(self.learning_rate), 0, 0, 0, 0, 1, 1, f(self.epsilon))
        return _AdaptiveConsts(_ADAPTIVE_KIND[self.kind], f(self.learning_rate), f(b1), f(1.0 - b1), f(b2), f(1.0 - b2),
                               f(1.0 - b1 ** t), f(1.0 - b2 ** t), f(self.epsilon))


def _f32_weights(name, weights):
    """The collaborator weights as the float32 values the reference's gradient
    multiplies by: a Python int / float beside a float32 array is rounded to
    float32 (np.float32: as it is).  Any other NumPy scalar would promote the
    gradient to float64 under NumPy >= 2, which is not implemented."""
    out = np.empty(len(weights), np.float32)
    for c, w in enumerate(weights):
        if isinstance(w, np.generic) and not isinstance(w, np.float32):
            raise _lib.CodecError(
                f"{name}: weight {c} is a {type(w).__name__}; with it NumPy >= 2 computes the reference's gradient "
                "in float64, which is not implemented -- pass Python floats (data_size / weight_total) or np.float32")
        if not isinstance(w, (int, float, np.float32)):
            raise _lib.CodecError(f"{name}: weight {c} must be a Python int or float or a np.float32")
        out[c] = np.float32(w)
    return out


def adaptive_step(hyper, steps_taken, xs, weights32, base, n, p, m, v, agg_out=None, delta_out=None, device=None):
    """One ofl_adaptive_step launch on the current stream: n elements of the
    float32 device tensors xs (collaborators, at most 128), base and the state
    p, m, v (updated in place; m may be None for adagrad), the step after
    `steps_taken`; agg_out = new p and delta_out = new p - base if given."""
    _check_collaborators(hyper.kind, len(xs), _ADAPTIVE_MAX_C)
    if len(xs) < 1 or len(weights32) != len(xs):
        raise _lib.CodecError(f"{hyper.kind}: one float32 weight per collaborator tensor, at least one")
    ptrs = _ptrs(xs)
    w32 = np.ascontiguousarray(weights32, np.float32)
    k = hyper.consts(steps_taken)
    _lib.check_agg(_lib.lib().ofl_adaptive_step(
        len(xs), ptrs.ctypes.data, w32.ctypes.data, base.data_ptr(), int(n), p.data_ptr(), _ptr(m), v.data_ptr(),
        ctypes.addressof(k), _ptr(agg_out), _ptr(delta_out), _stream(device)))


class _AdaptiveAggregation(_Plugin):
    """AdaptiveAggregation (core/adaptive_aggregation.py:16-113) with the
    optimiser's state on the device.  params: dict name -> float32 array, the
    parameters the optimiser owns (copied to the device; unlike the reference
    the caller's arrays are not updated in place).  model_interface is not
    offered: it needs the framework adapters to read a model's tensors.
    call() gives the reference's bits for float32 tensors and Python-float (or
    np.float32) weights; other NumPy weight types are refused (see
    _f32_weights)."""
    kind = None

    def __init__(self, *, params, agg_func=None, device=None, **hyper):
        self.hyper = AdaptiveHyper(self.kind, **hyper)
        if params is None:
            raise ValueError("Should provide params (model_interface is not supported)")
        self.default_agg_func = agg_func if agg_func is not None else WeightedAverage(device)
        self.device = resolve_device(device)
        self._shape, self._p, self._m, self._v = {}, {}, {}, {}
        self.current_step = {}
        for name, arr in params.items():
            a = np.asarray(arr)
            if a.dtype != np.float32:
                raise _lib.CodecError(f"{self.kind}: parameter {name!r} must be float32, not {a.dtype}")
            self._shape[name] = a.shape
            flat = np.ascontiguousarray(a).reshape(-1)
            with torch.cuda.device(self.device):
                self._p[name] = torch.from_numpy(flat.copy()).to(self.device)
                acc = self.hyper.initial_accumulator_value
                self._m[name] = torch.full_like(self._p[name], acc) if self.kind != "adagrad" else None
                self._v[name] = torch.full_like(self._p[name], acc)
            self.current_step[name] = 0

    @property
    def params(self):
        return self._shape.keys()

    def state(self, name):
        """Host copies of the device state of one parameter: p, m (None for
        adagrad), v in the parameter's shape, and the steps taken."""
        sh = self._shape[name]
        get = lambda t: None if t is None else t.cpu().numpy().reshape(sh)  # noqa: E731
        return {"params": get(self._p[name]), "first_moment": get(self._m[name]),
                "second_moment": get(self._v[name]), "step": self.current_step[name]}

    def set_state(self, name, first_moment=None, second_moment=None, step=None):
        """Overwrite parts of one parameter's state (a restored checkpoint):
        float32 arrays of the parameter's shape, the steps already taken."""
        for store, arr in ((self._m, first_moment), (self._v, second_moment)):
            if arr is None:
                continue
            a = np.asarray(arr)
            if a.dtype != np.float32 or a.shape != self._shape[name] or store[name] is None:
                raise _lib.CodecError(f"{self.kind}: state of {name!r} must be float32 of shape {self._shape[name]}")
            store[name] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).to(self.device)
        if step is not None:
            self.current_step[name] = int(step)

    def call(self, local_tensors, db_iterator, tensor_name, fl_round, tags):
        if tensor_name not in self._shape:
            return self.default_agg_func(local_tensors, db_iterator, tensor_name, fl_round, tags)
        base = None
        search_tag = "aggregated" if fl_round != 0 else "model"
        for record in db_iterator:
            if (record["round"] == fl_round and record["tensor_name"] == tensor_name
                    and search_tag in record["tags"] and "delta" not in record["tags"]):
                base = record["nparray"]
        if base is None:
            raise KeyError(f"There is no current global model in TensorDB for tensor name: {tensor_name}")
        arrs, shape, n = _f32_stack(self.kind, [x.tensor for x in local_tensors] + [base])
        if shape != self._shape[tensor_name]:
            raise _lib.CodecError(f"{self.kind}: {tensor_name!r} has shape {self._shape[tensor_name]}, not {shape}")
        w32 = _f32_weights(self.kind, [x.weight for x in local_tensors])
        if len(arrs) < 2:
            raise _lib.CodecError(f"{self.kind}: no tensors")
        _check_collaborators(self.kind, len(arrs) - 1, _ADAPTIVE_MAX_C)
        dev = self.device
        p = self._p[tensor_name]
        with torch.cuda.device(dev):
            if n:
                ts = _flat_to(arrs, dev)
                adaptive_step(self.hyper, self.current_step[tensor_name], ts[:-1], w32, ts[-1], n, p,
                              self._m[tensor_name], self._v[tensor_name], device=dev)
            self.current_step[tensor_name] += 1
            return p.cpu().numpy().reshape(shape)


class AdamAdaptiveAggregation(_AdaptiveAggregation):
    """adam_adaptive_aggregation.py:18-57 (NumPyAdam): AdamAdaptiveAggregation(*,
    params, agg_func=WeightedAverage(), learning_rate=0.01, betas=(0.9, 0.999),
    initial_accumulator_value=0.0, epsilon=1e-8, device=None)."""
    kind = "adam"


class YogiAdaptiveAggregation(_AdaptiveAggregation):
    """yogi_adaptive_aggregation.py (NumPyYogi): the arguments and defaults of
    AdamAdaptiveAggregation."""
    kind = "yogi"


class AdagradAdaptiveAggregation(_AdaptiveAggregation):
    """adagrad_adaptive_aggregation.py (NumPyAdagrad): AdagradAdaptiveAggregation(*,
    params, agg_func=WeightedAverage(), learning_rate=0.01,
    initial_accumulator_value=0.1, epsilon=1e-10, device=None); no betas."""
    kind = "adagrad"


class _RangeTable:
    """Element ranges [(start, count)] of an arena as the device tables the
    *_ranges and *_seeds entry points take: n ranges of `total` elements,
    start [n] and dst [n + 1] (the exclusive prefix of the counts)."""

    def __init__(self, ranges, device):
        counts = [c for _, c in ranges]
        self.n = len(ranges)
        self.total = int(sum(counts))
        self.start = torch.tensor([s for s, _ in ranges] or [0], dtype=torch.int64).to(device)
        self.dst = torch.from_numpy(np.cumsum([0] + counts).astype(np.int64)).to(device)

    @property
    def args(self):
        """(nranges, starts, dst, total), the order every entry point has them in."""
        return self.n, self.start.data_ptr(), self.dst.data_ptr(), self.total


# what RoundEnd._device_seeds sums: the weighted average's float64 delta, formed
# again from the collaborators, or another aggregate's arena (float64: agg - base)
_WavgSeeds = collections.namedtuple("_WavgSeeds", "w64 wsum fused")
_AggSeeds = collections.namedtuple("_AggSeeds", "agg is_f64 base")


class _LossyTail:
    """What follows the delta when the pipeline is a KCPipeline, SKCPipeline or
    STCPipeline: compress, decompress and apply_delta of every tensor.  The
    bytes are decoded straight after they are encoded and gzip is lossless, so
    decompress(compress(delta)) is the delta's labelling rule followed by the
    reference's key -> value replacement (kc_pipeline.py:79-83), and the new
    model is base + value_of(label(delta)) per element: one lossy.label_apply
    over value records, no rank array and no decoded delta (the ranks are
    written only where payloads are asked for).
      KC   k-means of the delta arena, one np.random seed per tensor
      SKC  top-k into a sparse arena, k-means of that (float64 centres)
      STC  top-k, the ternary rule as a record built from its statistics
    Tensors the device path does not take (n < n_clusters for KC / SKC, empty
    ones) go through the pipeline's own forward / backward on the host, with
    their delta in the dtype the reference computes it in."""

    def __init__(self, re, pipeline):
        self.re, self.pipeline = re, pipeline
        self.kind = "kc" if isinstance(pipeline, KCPipeline) else "skc" if isinstance(pipeline, SKCPipeline) else "stc"
        trs = pipeline.transformers
        self.gz = trs[-1]
        self.k = 0
        if self.kind != "stc":
            self.k = int(trs[-2].n_cluster)
            if not 1 <= self.k <= 8:
                raise _lib.CodecError(f"RoundEnd: n_clusters = {self.k}; label records need 1 <= k <= 8")
        # the reference clusters the delta in its own dtype; SKC's sparsifier emits float64
        self.value_f64 = self.kind == "skc" or re.aggregation in ("weighted_average", "geometric_median")
        take = (lambda n: n > 0) if self.kind == "stc" else (lambda n: n >= self.k)
        self.dev = [i for i, n in enumerate(re.numels) if take(n)]
        self.host = [i for i, n in enumerate(re.numels) if not take(n)]
        self.off = np.asarray([re.offsets[i] for i in self.dev], np.int64)
        self.num = np.asarray([re.numels[i] for i in self.dev], np.int64)
        self.ks = None if self.kind == "kc" else [_topk_count(int(n), pipeline.p) for n in self.num]
        hidx = [np.arange(re.offsets[i], re.offsets[i] + re.numels[i]) for i in self.host if re.numels[i]]
        self._hidx = torch.from_numpy(np.concatenate(hidx).astype(np.int64)).to(re.device) if hidx else None

    def _metadata(self, i, int_to_float, gz_md):
        shape = list(self.re.shapes[i])
        if self.kind == "kc":
            return [{"int_list": shape, "int_to_float": int_to_float}, gz_md]
        return [{"int_list": shape}, {"int_to_float": int_to_float}, gz_md]

    def _host_deltas(self, delta, src, xs, weights, base_arena):
        """The host-path tensors' deltas as the reference computes them, and
        their base: {i: (delta, base or None)}.  Weighted average: np.average
        itself on these few elements, minus the base in float64; geometric
        median: the float64 aggregate minus the base; otherwise the float32
        delta arena's elements."""
        re = self.re
        if self._hidx is None:
            return {i: (np.zeros(re.shapes[i], np.float32), None) for i in self.host}
        pick = lambda a: a.index_select(0, self._hidx)  # noqa: E731
        wavg = isinstance(src, _WavgSeeds)
        rows = ([pick(x) for x in xs] if wavg else [pick(delta)]) + ([pick(base_arena)] if base_arena is not None else [])
        rows = torch.stack(rows).cpu().numpy()
        agg64 = pick(src.agg).cpu().numpy() if not wavg and src.is_f64 else None
        res, o = {}, 0
        for i in self.host:
            n, shape = re.numels[i], re.shapes[i]
            part = lambda r: r[o:o + n].reshape(shape)  # noqa: E731
            base = part(rows[-1]) if base_arena is not None else None
            if wavg:
                d = np.average([part(rows[c]) for c in range(len(xs))], weights=weights, axis=0)
                d = d - base if base is not None else d
            elif agg64 is not None:
                d = part(agg64) - base if base is not None else part(agg64)
            else:
                d = part(rows[0])
            res[i] = (d, base)
            o += n
        return res

    def run(self, delta, src, xs, weights, base_arena, payloads, out):
        re, pipe = self.re, self.pipeline
        dev, T, nd = re.device, len(re.numels), len(self.dev)
        seeds = [None] * T
        draws = None
        if self.kind != "stc" and nd:  # what kmeans_ranks draws per tensor, in tensor order
            draws = np.random.randint(0, 2 ** 31 - 1, size=nd)
            for i, sd in zip(self.dev, draws):
                seeds[i] = int(sd)
        x, maps, ranks, r3 = delta, [], None, None
        if nd:
            if self.kind != "kc":
                x = re._empty_arena()
                st = lossy.sparsify_topk_batch(delta, self.off, self.num, self.ks, x)
            if self.kind == "stc":
                if not np.isfinite(st["abs_sum"]).all():
                    raise _lib.CodecError("stc: non-finite input")
                tm = [ternary_map(int(n), int(st["n_pos"][t]), int(st["n_neg"][t]), float(st["abs_sum"][t]))
                      for t, n in enumerate(self.num)]
                maps, r3 = [m for m, _ in tm], [r for _, r in tm]
                vrec = lossy.ternary_label_table(self.off, self.num, maps, r3, dev)
            else:
                vrec = lossy.LabelTable(nd, dev)
                ranks = re._empty_arena() if payloads else None
                uniq = lossy.kmeans_batch(x, self.off, self.num, self.k, n_init=self.k, seeds=draws,
                                          value_f64=self.value_f64, ranks_out=ranks, value_out=vrec)[3]
                maps = [{j: u for j, u in enumerate(uq)} for uq in uniq]
        # the host path: the pipeline's own forward and backward (nothing of `out` is written yet)
        result = [None] * T if payloads else None
        new_host = []
        for i, (d, base) in self._host_deltas(delta, src, xs, weights, base_arena).items():
            payload, md = pipe.forward(d)
            dec = pipe.backward(payload, [dict(m) for m in md])
            new_host.append(np.asarray(base + dec if base is not None else dec, np.float32).reshape(-1))
            if payloads:
                result[i] = (payload, md)
        if out is None:
            out = re._empty_arena()
        if nd:
            lossy.label_apply(x, vrec, base_arena, out)
        if self._hidx is not None:
            out.index_copy_(0, self._hidx, torch.from_numpy(np.concatenate(new_host)).to(dev))
        re._zero_gaps(out)
        if payloads and nd:
            if self.kind == "stc":
                ranks = lossy.ternary_ranks_batch(x, self.off, self.num, r3, re._empty_arena())
            for t, i in enumerate(self.dev):
                o, n = int(self.off[t]), int(self.num[t])
                payload, gz_md = self.gz.forward_device(ranks[o:o + n])
                result[i] = (payload, self._metadata(i, maps[t], gz_md))
        return out, result, seeds


_POINTS_MAX_C = 2048  # ofl_wavg_delta_points: collaborators of a 1-element tensor's pairwise sum


class WavgAccumulator:
    """RoundEnd.accumulator(): the weighted average taken one collaborator at
    a time.  add(arena, weight) folds one collaborator's arena into a float64
    sums arena (ofl_wavg_accumulate) and is done with it, so a round keeps
    one sums arena resident instead of every collaborator's; RoundEnd.finish
    divides, takes the delta and runs the rest of the round end.  The order of
    add() is the order of the float64 sum -- np.average's order over the
    collaborator axis -- so the caller adds in the collaborators' order and
    serialises the adds (one thread, one stream: the current one).  The
    1-element tensors, which NumPy sums pairwise, keep every collaborator's
    element in a small [C, nsingle] device table until finish()."""

    def __init__(self, re, sums):
        self.re = re
        self.sums = sums
        self.weights = []
        self.finished = False
        self._scratch = None   # add_upload's decode arena
        self._table = None     # [capacity, nsingle] float32: row c = collaborator c's 1-element tensors

    def _row(self, c):
        ns = len(self.re.single)
        if self._table is None or c >= self._table.shape[0]:
            grown = torch.empty((max(16, 2 * c), ns), dtype=torch.float32, device=self.re.device)
            if c:
                grown[:c].copy_(self._table[:c])
            self._table = grown
        return self._table[c]

    def add(self, arena, weight):
        """Fold one collaborator in: arena (this layout, float32, on the
        device; free to reuse once the current stream has passed this call)
        and its weight (as run() takes them, not normalised)."""
        re = self.re
        if self.finished:
            raise _lib.CodecError("accumulator: add() after finish()")
        re._check_arena(arena)
        try:
            w = float(np.asarray(weight, np.float64).reshape(()))
        except (TypeError, ValueError) as e:
            raise _lib.CodecError(f"accumulator: weight {weight!r} is not a number") from e
        if np.result_type(np.float32, np.asarray(weight).dtype) != np.float64:
            _f64_weights(self.weights + [weight], len(self.weights) + 1)  # run()'s rule on the weights so far
        c = len(self.weights)
        if re.single and c >= _POINTS_MAX_C:
            raise _lib.CodecError(f"accumulator: at most {_POINTS_MAX_C} collaborators with 1-element tensors")
        with torch.cuda.device(re.device):
            _lib.check_agg(_lib.lib().ofl_wavg_accumulate(arena.data_ptr(), w, 1 if c == 0 else 0, re.arena_numel,
                                                          self.sums.data_ptr(), _stream(re.device)))
            if re.single:
                torch.index_select(arena, 0, re._single_idx, out=self._row(c))
        self.weights.append(weight)

    def add_upload(self, items, weight, lossless=False, delta=True, base_arena=None):
        """re.ingest(items, ...) into this accumulator's own scratch arena,
        then add(that, weight): one collaborator's upload as it arrives."""
        if self.finished:
            raise _lib.CodecError("accumulator: add_upload() after finish()")
        self._scratch = self.re.ingest(items, lossless=lossless, delta=delta, base_arena=base_arena, out=self._scratch)
        self.add(self._scratch, weight)


class RoundEnd:
    """Aggregator._prepare_trained for a whole model update (aggregator.py:780-865).

    pipeline: an openfl_amd EdenPipeline (its n_bits, dim_threshold and
    seed_mode apply), or a KCPipeline, SKCPipeline or STCPipeline (_LossyTail:
    n_clusters <= 8; fused= does not apply; run()'s third value is then the
    list of k-means seeds drawn, None where none was; a non-finite delta
    raises CodecError before `out` is written); shapes: the model's tensor shapes in the aggregator's
    order.  Tensors live in flat float32 arenas, tensor i at offsets[i]
    (64-element aligned); arena() / pack() / view() make and read them.
    fused (default): without agg_out and with at most 16 collaborators the
    large slices' first encode pass computes the delta from the collaborator
    arenas itself (ofl_eden_encode_wavg) instead of reading a delta arena
    the averaging kernel wrote -- same bytes, 8 B/element less HBM traffic.
    aggregation: "weighted_average" (default), "median" (np.median per
    element, at most 128 collaborators, run()'s weights may be None and its
    agg_out is float32) or "geometric_median" (Weiszfeld per tensor with the
    reference's defaults, at most 16 collaborators, agg_out float64).  The two
    robust aggregators write the delta arena with their own kernels, take the
    seeds from it (ofl_agg_delta_seeds) and are never fused; everything after
    the seeds is the same code.
    aggregation "adam", "yogi" or "adagrad" (ADAPTIVE_AGGREGATIONS): the FedOpt
    server optimisers (AdaptiveAggregation over NumPyAdam / NumPyYogi /
    NumPyAdagrad), at most 128 collaborators, agg_out float32.  optimizer: a
    dict of the optimiser's hyper-parameters (learning_rate, betas,
    initial_accumulator_value, epsilon; the reference's defaults and checks).
    Every tensor of the layout is optimised -- what a plan's model_interface
    gives, whose whole tensor dict is the optimiser's params; leaving single
    tensors to another aggregation function is not offered here (the plugins
    do it).  The state (parameters, first and second moment, step count)
    lives in arenas of this layout: init_optimizer(params_arena) before the
    first run(), optimizer_state() to read it.  run() needs base_arena (the
    gradient is formed against it), takes one ofl_adaptive_step over the
    arena, then the seeds from the float32 delta as the median does; never
    fused.  The aggregate is the reference's bit for bit for Python-float (or
    np.float32) weights; other NumPy weight types are refused.
    """

    def __init__(self, pipeline, shapes, device=None, fused=True, aggregation="weighted_average", optimizer=None):
        if aggregation not in AGGREGATIONS + ADAPTIVE_AGGREGATIONS:
            raise _lib.CodecError(
                f"aggregation must be one of {AGGREGATIONS + ADAPTIVE_AGGREGATIONS}, not {aggregation!r}")
        self.aggregation = aggregation
        if aggregation in ADAPTIVE_AGGREGATIONS:
            self._hyper = AdaptiveHyper(aggregation, **(optimizer or {}))
        elif optimizer is not None:
            raise _lib.CodecError(f"optimizer= belongs to the aggregations {ADAPTIVE_AGGREGATIONS}")
        self._opt = None   # (p, m, v) arenas after init_optimizer
        self._opt_step = 0
        is_lossy = isinstance(pipeline, (KCPipeline, SKCPipeline, STCPipeline))
        tr = pipeline.transformers[0]
        self.transformer = tr
        self.device = resolve_device(device) if device is not None else (tr.device if is_lossy else tr.eden.device)
        self.shapes = [tuple(int(d) for d in s) for s in shapes]
        self.numels = [int(np.prod(s, dtype=np.int64)) for s in self.shapes]
        self.offsets, acc = [], 0
        for n in self.numels:
            self.offsets.append(acc)
            acc += (n + _ALIGN - 1) // _ALIGN * _ALIGN
        self.arena_numel = max(acc, 1)
        # the alignment padding between tensors (and the arena's tail): zeroed
        # in every output arena, so it is the same whichever path ran
        gaps = [np.arange(o + n, o + (n + _ALIGN - 1) // _ALIGN * _ALIGN) for o, n in zip(self.offsets, self.numels)]
        gaps.append(np.arange(acc, self.arena_numel))
        gap_idx = np.concatenate(gaps).astype(np.int64) if gaps else np.zeros(0, np.int64)
        self._gap_idx = torch.from_numpy(gap_idx).to(self.device) if gap_idx.size else None
        self.single = [i for i, n in enumerate(self.numels) if n == 1]
        self._ws = _Scratch(self.device)
        # what follows the delta: _tail(delta, seed source, collaborators, weights, base, payloads, out)
        if is_lossy:
            self.fused = False
            self._lossy = _LossyTail(self, pipeline)
            self._tail = self._lossy.run
        else:
            self._lossy = None
            self._init_eden(tr, fused)
            self._tail = self._eden_tail
        # pinned [collaborator pointers | weights | draws], reused after _args_done, and its device copy
        self._host_args = self._dev_args = self._args_done = None
        # geometric median: the chunk table of this layout, per-tensor state and
        # (without agg_out) the float64 aggregate the delta and seeds come from
        self._gm = _GmLayout(self.offsets, self.numels, self.device) if aggregation == "geometric_median" else None
        self._gm_agg = None
        # ingest(): the pipeline whose payloads it decodes, its pinned staging per
        # payload kind (reused once _ingest_done has passed) and its decode arena
        self.pipeline = pipeline
        self._ingest_stage, self._ingest_done, self._ingest_tmp = {}, None, None
        self._single_idx = None   # accumulator(): the 1-element tensors' offsets on the device

    def _init_eden(self, tr, fused):
        """The Eden back end's plan and device tables (_device_seeds, _encode_apply)."""
        self.dim_threshold = tr.dim_threshold
        self.seed_mode = tr.seed_mode
        self.n_bits = tr.eden.nbits
        self.big = [i for i, n in enumerate(self.numels) if n > self.dim_threshold]
        self._big_slot = {i: t for t, i in enumerate(self.big)}
        self.plan = EdenPlan([self.numels[i] for i in self.big], self.n_bits,
                             elem_offsets=[self.offsets[i] for i in self.big]) if self.big else None
        self._codec_ws = None
        # tensors the codec does not touch (small, <= dim_threshold): their
        # apply_delta runs on these ranges (device tables)
        rest = [(self.offsets[i], n) for i, n in enumerate(self.numels) if 0 < n <= self.dim_threshold]
        self._rest = _RangeTable(rest, self.device)
        # seed ranges (a prefix per tensor in fast mode, all of it in reference
        # mode) as device tables: the seeds are computed without a host round trip
        T = len(self.numels)
        counts = [min(n, _FAST_SEED_PREFIX) if self.seed_mode == "fast" else n for n in self.numels]
        self._seed = _RangeTable(list(zip(self.offsets, counts)), self.device)
        self._seed_single = torch.tensor([1 if n == 1 else 0 for n in self.numels] or [0], dtype=torch.int32).to(self.device)
        self._seed_sums = torch.empty(max(T, 1), dtype=torch.float64, device=self.device)
        self._seeds = torch.empty(max(T, 1), dtype=torch.int32, device=self.device)
        self._packed = torch.empty(max(self._seed.total, 1), dtype=torch.float64, device=self.device)
        self._big_idx = torch.tensor(self.big or [0], dtype=torch.int64).to(self.device)
        # fused round-end encode (ofl_eden_encode_wavg): the large slices' row
        # pass computes the delta from the collaborators' arenas itself, so the
        # delta arena is written only where something else reads it -- the
        # tensors the codec does not touch and the slices of <= 2^15 elements
        self.fused = bool(fused) and self.plan is not None and self.aggregation == "weighted_average"
        fz = list(rest)
        for t, i in enumerate(self.big):
            _, lens = slice_plan(self.numels[i])
            xo = self.offsets[i]
            for P, ln in zip(self.plan.dims[t], lens):
                if P <= _ROW_TILE and ln > 0:
                    fz.append((xo, ln))
                xo += ln
        self._fz = _RangeTable(sorted(fz), self.device)

    # -- arenas --
    def arena(self):
        return torch.zeros(self.arena_numel, dtype=torch.float32, device=self.device)

    def pack(self, arrays):
        a = self.arena()
        for i, x in enumerate(arrays):
            x = np.asarray(x, np.float32).reshape(-1)
            if x.size != self.numels[i]:
                raise _lib.CodecError(f"tensor {i}: {x.size} elements, expected {self.numels[i]}")
            a[self.offsets[i]:self.offsets[i] + x.size] = torch.from_numpy(x).to(self.device)
        return a

    def view(self, arena, i):
        return arena[self.offsets[i]:self.offsets[i] + self.numels[i]].view(self.shapes[i])

    # -- a collaborator's upload into an arena --
    def ingest(self, items, lossless=False, delta=True, base_arena=None, out=None):
        """One collaborator's upload, as the aggregator receives it, decoded
        into a device arena of this layout (Aggregator._process_named_tensor,
        aggregator.py:690-778, for every tensor of the model at once).
        items: one (payload bytes, metadata list) per tensor in layout order --
        NamedTensor.data_bytes and transformer_metadata; the metadata may be
        dicts and lists or the protobuf containers (protocols.
        transformer_metadata_of).  Unlike TransformationPipeline.backward,
        which pops its metadata list, ingest leaves items as they are.
        lossless=True: every payload is NoCompressionPipeline's (raw float32
        bytes + int_list, the `compressed` tag); lossless=False: every payload
        is this RoundEnd's pipeline's (`lossy_compressed`).  delta=True: the
        result is base_arena + decoded, a float32 add (TensorCodec.apply_delta),
        and base_arena is required.  -> `out` (default: a new arena; may be
        base_arena): per tensor the bits of pipe.backward(payload, metadata)
        (+ base), the alignment gaps zero.
        Eden: the tensors above dim_threshold are decoded as one batch with this
        RoundEnd's plan (planes gathered into pinned staging, one H2D; the
        decode adds the base itself), so their metadata must name the layout's
        slice plan, as every conforming encoder's does.  KC / SKC / STC: one
        device inflate with the fused LUT per tensor, into a decode arena of
        this instance, so `out` is written only once everything has decoded.
        Every check of the items (count, int_list against the layout, payload
        lengths, Eden metadata) raises CodecError naming the tensor before
        `out` is written or anything is launched.
        Not thread-safe per RoundEnd: it uses the instance's staging and
        decode arena, and the current stream."""
        dev = resolve_device(getattr(self, "device", None))
        items = list(items)
        T = len(self.numels)
        if len(items) != T:
            raise _lib.CodecError(f"ingest: {len(items)} items, the layout has {T} tensors")
        if delta and base_arena is None:
            raise _lib.CodecError("ingest: delta=True needs base_arena")
        for a in (base_arena, out):
            if a is not None:
                self._check_arena(a)
        kind = "raw" if lossless else "eden" if self._lossy is None else "lossy"
        bufs = self._ingest_check(items, kind)
        with torch.cuda.device(dev):
            if out is None:
                out = self._empty_arena()
            getattr(self, "_ingest_" + kind)(items, bufs, base_arena if delta else None, out)
            self._zero_gaps(out)
        return out

    def _ingest_check(self, items, kind):
        """ingest's checks of the items, all before anything is written ->
        the payloads as uint8 arrays (views of the bytes)."""
        nmd = 1 if kind != "lossy" else 2 if self._lossy.kind == "kc" else 3
        inflated = set(self._inflated()) if kind == "lossy" else ()
        bufs = []
        for i, item in enumerate(items):
            n = self.numels[i]
            try:
                payload, mds = item
                buf = np.frombuffer(payload, np.uint8)
                if len(mds) != nmd:
                    raise _lib.CodecError(f"tensor {i}: {len(mds)} metadata entries, expected {nmd}")
                shape = tuple(int(d) for d in mds[0]["int_list"])
            except _lib.CodecError:
                raise
            except (TypeError, ValueError, KeyError, IndexError) as e:
                raise _lib.CodecError(f"tensor {i}: not a (payload bytes, metadata list) item: {e!r}") from e
            if shape != self.shapes[i]:
                raise _lib.CodecError(f"tensor {i}: int_list {list(shape)}, the layout has {list(self.shapes[i])}")
            if kind == "lossy":
                if i in inflated and buf.size < 18:
                    raise _lib.CodecError(f"tensor {i}: payload has {buf.size} bytes, a gzip member has at least 18")
            elif kind == "eden" and n > self.dim_threshold:
                t = self._big_slot[i]
                try:
                    m = dict(mds[0]["int_to_float"])
                    total = int(m[1])
                    dims = [int(m[k + 1]) for k in range(2, max(m) + 1, 2)]
                    float(m[0]), [float(m[k]) for k in range(2, max(m) + 1, 2)]
                except (TypeError, ValueError, KeyError) as e:
                    raise _lib.CodecError(f"tensor {i}: bad Eden metadata: {e!r}") from e
                if total != n or dims != self.plan.dims[t]:
                    raise _lib.CodecError(f"tensor {i}: Eden metadata names total_dim {total} in slices {dims}; this "
                                          f"layout's slice plan is {n} in {self.plan.dims[t]}")
                if buf.size < self.plan.planes_nbytes[t]:
                    raise _lib.CodecError(f"tensor {i}: payload has {buf.size} bytes, the planes take "
                                          f"{self.plan.planes_nbytes[t]}")
            elif buf.size != 4 * n:
                raise _lib.CodecError(f"tensor {i}: payload has {buf.size} bytes, {n} float32 values take {4 * n}")
            bufs.append(buf)
        return bufs

    def _raw_runs(self, raw):
        """Where raw float32 tensors wait in pinned staging: neighbours in the
        arena keep their spacing, so a run of them is one H2D.  raw: tensor
        indices in order -> ({tensor: staging element offset}, [(arena start,
        staging start, elements)], staging elements)."""
        is_raw = set(raw)
        at, runs, acc, open_run = {}, [], 0, False
        for i, n in enumerate(self.numels):
            if n == 0:
                continue
            if i not in is_raw:
                open_run = False
                continue
            if not open_run:
                runs.append([self.offsets[i], acc, 0])
                open_run = True
            a0, s0, _ = runs[-1]
            at[i] = s0 + self.offsets[i] - a0
            runs[-1][2] = self.offsets[i] + n - a0
            acc = (s0 + runs[-1][2] + _ALIGN - 1) // _ALIGN * _ALIGN
        return at, [tuple(r) for r in runs], acc

    def _ingest_staging(self, kind, raw, extra_bytes=0):
        """The pinned staging of one payload kind: [raw tensors as _raw_runs
        places them | extra bytes], made once.  The previous ingest's copies
        have left it when this returns."""
        st = self._ingest_stage.get(kind)
        if st is None:
            at, runs, numel = self._raw_runs(raw)
            extra_at = (4 * numel + 255) // 256 * 256
            host = torch.empty(max(extra_at + extra_bytes, 1), dtype=torch.uint8).pin_memory()
            st = self._ingest_stage[kind] = {"at": at, "runs": runs, "host": host, "extra_at": extra_at}
        if self._ingest_done is not None:
            self._ingest_done.synchronize()
        return st

    def _stage_raw(self, st, tensors, srcs, dst):
        """Raw float32 tensors (host addresses srcs) through the staging into the
        arena dst: the native multi-copy, then one H2D per run."""
        base = st["host"].data_ptr()
        _copy_many([base + 4 * st["at"][i] for i in tensors], srcs, [4 * self.numels[i] for i in tensors])
        f32 = st["host"][:st["extra_at"]].view(torch.float32)
        for a0, s0, n in st["runs"]:
            dst[a0:a0 + n].copy_(f32[s0:s0 + n], non_blocking=True)

    def _ingest_sent(self):
        if self._ingest_done is None:
            self._ingest_done = torch.cuda.Event()
        self._ingest_done.record()

    def _decode_arena(self):
        if self._ingest_tmp is None:
            self._ingest_tmp = self._empty_arena()
        return self._ingest_tmp

    def _ingest_raw(self, items, bufs, base, out):
        """NoCompressionPipeline's payloads: staged at the arena's layout, one H2D."""
        raw = [i for i, n in enumerate(self.numels) if n]
        st = self._ingest_staging("raw", raw)
        dst = out if base is None else self._decode_arena()
        self._stage_raw(st, raw, [bufs[i].ctypes.data for i in raw], dst)
        self._ingest_sent()
        if base is not None:
            _lib.check_agg(_lib.lib().ofl_apply_delta(base.data_ptr(), dst.data_ptr(), self.arena_numel, out.data_ptr(),
                                                      _stream(self.device)))

    def _ingest_eden(self, items, bufs, base, out):
        """EdenPipeline's payloads: the big tensors' planes, scales and seeds in
        one H2D and one batch decode (which adds the base); the rest are raw."""
        dev, p = self.device, self.plan
        raw = [i for i, n in enumerate(self.numels) if 0 < n <= self.dim_threshold]
        off_scales = (p.planes_bytes + 255) // 256 * 256 if p is not None else 0
        off_seeds = (off_scales + 4 * p.n_slices + 255) // 256 * 256 if p is not None else 0
        nbytes = off_seeds + 4 * len(self.big)
        st = self._ingest_staging("eden", raw, nbytes)
        if raw:
            dst = out if base is None else self._decode_arena()
            self._stage_raw(st, raw, [bufs[i].ctypes.data for i in raw], dst)
        if p is not None:
            host = st["host"][st["extra_at"]:st["extra_at"] + nbytes]
            hp = host.data_ptr()
            _copy_many([hp + p.planes_offsets[t] for t in range(len(self.big))],
                       [bufs[i].ctypes.data for i in self.big], list(p.planes_nbytes))
            ha = host.numpy()
            scales = ha[off_scales:off_scales + 4 * p.n_slices].view(np.float32)
            seeds = ha[off_seeds:off_seeds + 4 * len(self.big)].view(np.uint32)
            for t, i in enumerate(self.big):
                m = dict(items[i][1][0]["int_to_float"])
                fs = p.first_slice[t]
                seeds[t] = int(m[0]) & 0xFFFFFFFF
                scales[fs:fs + len(p.dims[t])] = [m[2 + 2 * k] for k in range(len(p.dims[t]))]
            d = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            d.copy_(host, non_blocking=True)
            if self._codec_ws is None or self._codec_ws.numel() < p.ws_bytes:
                self._codec_ws = torch.empty(max(p.ws_bytes, 256), dtype=torch.uint8, device=dev)
            p.decode(d[:max(p.planes_bytes, 1)], d[off_seeds:].view(torch.int32),
                     d[off_scales:off_scales + 4 * p.n_slices].view(torch.float32), out, self._codec_ws, base=base)
        self._ingest_sent()
        if raw and base is not None:
            _lib.check_agg(_lib.lib().ofl_apply_delta_ranges(base.data_ptr(), dst.data_ptr(), out.data_ptr(),
                                                             *self._rest.args, _stream(dev)))

    def _inflated(self):
        """The tensors whose payloads the lossy pipeline's backward inflates on
        the device (its host path takes the others: n < n_clusters, empty ones,
        and everything with the host gzip backend)."""
        return self._lossy.dev if self._lossy.gz.backend == "device" else []

    def _ingest_lossy(self, items, bufs, base, out):
        """KC / SKC / STC payloads: the pipeline's device backward per tensor
        (inflate with the fused LUT) straight into the tensor's place in the
        decode arena; the tensors on the pipeline's host path through its own
        backward, staged like raw ones.  `out` is written from the decode
        arena once every tensor has decoded."""
        dev = self.device
        inflated = self._inflated()
        host_path = [i for i, n in enumerate(self.numels) if n and i not in set(inflated)]
        st = self._ingest_staging("lossy", host_path)
        dst = self._decode_arena()
        where = 0 if self._lossy.kind == "kc" else 1
        for i in inflated:
            o, n = self.offsets[i], self.numels[i]
            m = items[i][1][where]["int_to_float"]
            try:
                lossy.gunzip_device(items[i][0], dst[o:o + n].view(torch.uint8),
                                    lut=lossy.lut_tables([0], [n], [m], dev), expect_bytes=4 * n)
            except (_lib.CodecError, EOFError, OSError, zlib.error) as e:   # the last three: the host fallback's
                raise _lib.CodecError(f"tensor {i}: {e}") from e
        if host_path:
            dec = [np.ascontiguousarray(self.pipeline.backward(items[i][0], list(items[i][1])), np.float32).reshape(-1)
                   for i in host_path]
            for i, y in zip(host_path, dec):
                if y.size != self.numels[i]:
                    raise _lib.CodecError(f"tensor {i}: decodes to {y.size} elements, expected {self.numels[i]}")
            self._stage_raw(st, host_path, [y.ctypes.data for y in dec], dst)
        self._ingest_sent()
        if base is not None:
            _lib.check_agg(_lib.lib().ofl_apply_delta(base.data_ptr(), dst.data_ptr(), self.arena_numel, out.data_ptr(),
                                                      _stream(dev)))
        else:
            out[:self.arena_numel].copy_(dst)

    # -- the weighted average one collaborator at a time --
    def accumulator(self, sums=None):
        """A WavgAccumulator for one round of this layout (aggregation
        "weighted_average" only): acc.add(arena, weight) or acc.add_upload(items,
        weight, ...) per collaborator, in the collaborators' order, then
        finish(acc, ...).  sums: the float64 arena (arena_numel elements) the
        running sums and then the average live in; default: a new one."""
        dev = resolve_device(getattr(self, "device", None))
        if self.aggregation != "weighted_average":
            raise _lib.CodecError(f"accumulator() is the weighted average's; this RoundEnd aggregates by "
                                  f"{self.aggregation!r}")
        if sums is None:
            sums = torch.empty(self.arena_numel, dtype=torch.float64, device=dev)
        elif not (sums.is_cuda and sums.dtype == torch.float64 and sums.is_contiguous()
                  and sums.numel() >= self.arena_numel):
            raise _lib.CodecError("sums must be a contiguous float64 device tensor of arena_numel elements")
        if self.single and self._single_idx is None:
            self._single_idx = torch.tensor([self.offsets[i] for i in self.single], dtype=torch.int64).to(dev)
        return WavgAccumulator(self, sums)

    def finish(self, acc, base_arena=None, agg_out=None, payloads=True, out=None):
        """The round end of what acc has accumulated: exactly what run(arenas,
        weights, base_arena, agg_out, payloads, out) returns for the arenas and
        weights added, in that order -- the new model, the payloads and their
        metadata, the seeds and the np.random draws.  The sums are divided by
        the weights' sum in place (ofl_wavg_finish, which also writes the
        float32 delta), the 1-element tensors are redone in NumPy's pairwise
        order from acc's table (ofl_wavg_delta_points), and the seeds come from
        the float64 average minus the base (ofl_agg_delta_seeds), the route the
        geometric median takes; never fused.  agg_out (float64, arena_numel
        elements) receives the average; acc.sums holds it anyway.  An
        accumulator is finished once.  All errors are raised before anything
        is launched or drawn from np.random."""
        dev = resolve_device(getattr(self, "device", None))
        if not isinstance(acc, WavgAccumulator) or acc.re is not self:
            raise _lib.CodecError("finish() takes an accumulator() of this RoundEnd")
        if acc.finished:
            raise _lib.CodecError("accumulator: finish() after finish()")
        if not acc.weights:
            raise _lib.CodecError("accumulator: finish() without an add()")
        if base_arena is not None:
            self._check_arena(base_arena)
        if agg_out is not None and not (agg_out.dtype == torch.float64 and agg_out.numel() >= self.arena_numel):
            raise _lib.CodecError("agg_out must be float64 with arena_numel elements")
        w64 = _f64_weights(acc.weights, len(acc.weights))
        wsum = self._wsum(w64)
        acc.finished = True
        L = _lib.lib()
        with torch.cuda.device(dev):
            delta = self._empty_arena()
            _lib.check_agg(L.ofl_wavg_finish(acc.sums.data_ptr(), wsum, _ptr(base_arena), self.arena_numel, None,
                                             delta.data_ptr(), _stream(dev)))
            if self.single:
                ns, C = len(self.single), len(w64)
                rows = [acc._table[c] for c in range(C)]
                b1 = base_arena.index_select(0, self._single_idx) if base_arena is not None else None
                a1 = torch.empty(ns, dtype=torch.float64, device=dev)
                d1 = torch.empty(ns, dtype=torch.float32, device=dev)
                _points_launch(rows, w64, wsum, b1, np.arange(ns), a1, d1, dev, self._ws)
                acc.sums.index_copy_(0, self._single_idx, a1)
                delta.index_copy_(0, self._single_idx, d1)
            if agg_out is not None and agg_out.data_ptr() != acc.sums.data_ptr():
                agg_out[:self.arena_numel].copy_(acc.sums[:self.arena_numel])
            return self._tail(delta, _AggSeeds(acc.sums, 1, base_arena), [], acc.weights, base_arena, payloads, out)

    # -- the optimiser's state (aggregation "adam" / "yogi" / "adagrad") --
    def init_optimizer(self, params_arena):
        """Start the optimiser from a copy of params_arena (this layout): first
        and second moment filled with initial_accumulator_value, no steps taken."""
        if self.aggregation not in ADAPTIVE_AGGREGATIONS:
            raise _lib.CodecError(f"aggregation {self.aggregation!r} has no optimizer")
        self._check_arena(params_arena)
        with torch.cuda.device(self.device):
            p = params_arena[:self.arena_numel].to(self.device, copy=True)
            acc = self._hyper.initial_accumulator_value
            m = torch.full_like(p, acc) if self.aggregation != "adagrad" else None
            self._opt = (p, m, torch.full_like(p, acc))
        self._opt_step = 0

    def optimizer_state(self):
        """The live state arenas (not copies) and the steps taken:
        {"params", "first_moment" (None for adagrad), "second_moment", "step"}."""
        if self._opt is None:
            raise _lib.CodecError("init_optimizer(params_arena) has not been called")
        p, m, v = self._opt
        return {"params": p, "first_moment": m, "second_moment": v, "step": self._opt_step}

    def _wsum(self, w64):
        sums = {weight_sum(w64, d) for d in {len(s) for s in self.shapes}}
        if len(sums) != 1:
            raise _lib.CodecError("weight sums differ between tensor ranks")
        s = sums.pop()
        if s == 0.0:
            raise ZeroDivisionError("Weights sum to zero, can't be normalized")
        return s

    def run(self, collab_arenas, weights, base_arena=None, agg_out=None, payloads=True, out=None):
        """collab_arenas: one float32 device arena per collaborator (this
        layout); weights: per collaborator; base_arena: the previous model
        (None: no base, the delta is the average).  Writes the new model
        into `out` (default: a new arena; may be base_arena) and, if given,
        the float64 average into agg_out (arena_numel elements).  With
        aggregation "median" the weights are ignored (may be None) and agg_out
        is float32; with "geometric_median" agg_out is float64 and is written
        inside the tensors only.  With "adam", "yogi" or "adagrad" the weights
        are Python floats (or np.float32), base_arena is required, agg_out is
        float32 (the parameters after the step) and the step count rises by one.
        -> (new model arena, [(payload bytes, [metadata])] per tensor or None,
        seeds: a list with payloads, else the device int32 tensor -- without
        payloads nothing synchronises with the host).  With a lossy pipeline
        the seeds are always the list of k-means seeds drawn (None per tensor
        where none was) and the k-means synchronises."""
        xs = list(collab_arenas)
        for x in xs + ([base_arena] if base_arena is not None else []):
            self._check_arena(x)
        f32_agg = self.aggregation == "median" or self.aggregation in ADAPTIVE_AGGREGATIONS
        agg_dtype = torch.float32 if f32_agg else torch.float64
        if agg_out is not None and not (agg_out.dtype == agg_dtype and agg_out.numel() >= self.arena_numel):
            raise _lib.CodecError(f"agg_out must be {str(agg_dtype)[6:]} with arena_numel elements")
        family = self.aggregation if self.aggregation in AGGREGATIONS else "adaptive"
        with torch.cuda.device(self.device):
            # 1. the aggregate and its delta rounded to float32, by the aggregation's kernels
            delta, seed_source = getattr(self, "_delta_" + family)(xs, weights, base_arena, agg_out)
            # what follows is the pipeline's: Eden -- 2. the seeds, 3. encode, (payloads), decode in
            # place, apply; KC / SKC / STC -- _LossyTail
            return self._tail(delta, seed_source, xs, weights, base_arena, payloads, out)

    def _eden_tail(self, delta, seed_source, xs, weights, base_arena, payloads, out):
        wavg = self._device_seeds(seed_source, xs, base_arena)
        return self._encode_apply(delta, base_arena, payloads, out, wavg)

    def _zero_gaps(self, out):
        if self._gap_idx is not None:
            out.index_fill_(0, self._gap_idx, 0.0)

    def _check_arena(self, x):
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() >= self.arena_numel):
            raise _lib.CodecError("arenas must be contiguous float32 device tensors of arena_numel elements")

    def _empty_arena(self):
        return torch.empty(self.arena_numel, dtype=torch.float32, device=self.device)

    # -- step 1 of run() per family -> (float32 delta arena, the seeds' source); all raise before the draws --
    def _delta_weighted_average(self, xs, weights, base_arena, agg_out):
        """average + delta in float64, the delta rounded to float32 -- fused:
        only on the ranges the large slices' encode does not compute."""
        dev = self.device
        w64 = _f64_weights(weights, len(xs))
        wsum = self._wsum(w64)
        fused = self.fused and agg_out is None and len(xs) <= 16
        delta = self._empty_arena()
        if agg_out is None and len(xs) > 16:  # running sums between chained launches
            agg_out = torch.empty(self.arena_numel, dtype=torch.float64, device=dev)
        if fused:
            ptrs = _ptrs(xs)
            _lib.check_agg(_lib.lib().ofl_wavg_delta32_ranges(
                len(xs), ptrs.ctypes.data, w64.ctypes.data, wsum, _ptr(base_arena), *self._fz.args, delta.data_ptr(),
                _stream(dev)))
        else:
            _wavg_launch(xs, w64, wsum, base_arena, self.arena_numel, agg=agg_out, delta32=delta, device=dev)
        if self.single:
            _points_launch(xs, w64, wsum, base_arena, [self.offsets[i] for i in self.single], agg_out, delta, dev,
                           self._ws)
        return delta, _WavgSeeds(w64, wsum, fused)

    def _delta_median(self, xs, weights, base_arena, agg_out):
        """elementwise over the whole arena; the float32 delta it writes is the
        array the seed formula sums."""
        delta = self._empty_arena()
        _median_launch(xs, base_arena, self.arena_numel, med=agg_out, delta=delta, device=self.device)
        return delta, _AggSeeds(delta, 0, None)

    def _delta_geometric_median(self, xs, weights, base_arena, agg_out):
        """Weiszfeld per tensor; the seeds come from generate_delta of the
        float64 aggregate: agg - base in float64."""
        _check_collaborators("geometric_median", len(xs), _GMEDIAN_MAX_C)
        w0 = _gm_start_weights(weights, len(xs))
        delta = self._empty_arena()
        if agg_out is None:
            if self._gm_agg is None:
                self._gm_agg = torch.zeros(self.arena_numel, dtype=torch.float64, device=self.device)
            agg_out = self._gm_agg
        self._gm.launch(xs, w0, 4, 1e-5, 1e-6, base_arena, agg=agg_out, delta32=delta, device=self.device)
        return delta, _AggSeeds(agg_out, 1, base_arena)

    def _delta_adaptive(self, xs, weights, base_arena, agg_out):
        """one elementwise step over the whole arena (in the alignment gaps
        everything is zero: a zero gradient); the float32 delta it writes is
        generate_delta of two float32 arrays."""
        if self._opt is None:
            raise _lib.CodecError(f"{self.aggregation}: call init_optimizer(params_arena) before run()")
        if base_arena is None:
            raise _lib.CodecError(f"{self.aggregation}: base_arena is required, the gradient is formed against it")
        _check_collaborators(self.aggregation, len(xs), _ADAPTIVE_MAX_C)
        if weights is None or len(weights) != len(xs) or not xs:
            raise _lib.CodecError("one weight per collaborator tensor")
        w32 = _f32_weights(self.aggregation, list(weights))
        delta = self._empty_arena()
        p, m, v = self._opt
        adaptive_step(self._hyper, self._opt_step, xs, w32, base_arena, self.arena_numel, p, m, v, agg_out=agg_out,
                      delta_out=delta, device=self.device)
        self._opt_step += 1
        return delta, _AggSeeds(delta, 0, None)

    def _device_seeds(self, src, xs, base_arena):
        """Step 2 of run(), into self._seeds without a host round trip: serial
        sums of the delta on the seed ranges, CPython's float hash, one
        np.random draw per tensor in order (drawn here).  -> (device args,
        collaborators, weight sum) for the fused encode, else None."""
        L = _lib.lib()
        T, C = len(self.numels), len(xs)
        draws = np.random.randint(1, 2 ** 16, size=T).astype(np.int64) if T else np.zeros(0, np.int64)
        out = self._seeds.data_ptr(), self._seed_sums.data_ptr(), self._packed.data_ptr(), _stream(self.device)
        if isinstance(src, _AggSeeds):
            dp = self._stage_args([draws])
            _lib.check_agg(L.ofl_agg_delta_seeds(src.agg.data_ptr(), src.is_f64, _ptr(src.base), *self._seed.args, dp,
                                                 *out))
            return None
        dp = self._stage_args([_ptrs(xs).view(np.int64), src.w64.view(np.int64), draws])
        _lib.check_agg(L.ofl_wavg_delta_seeds(
            C, dp, dp + 8 * C, src.wsum, _ptr(base_arena), T, self._seed.start.data_ptr(), self._seed.dst.data_ptr(),
            self._seed_single.data_ptr(), self._seed.total, dp + 16 * C, *out))
        return (dp, C, src.wsum) if src.fused else None

    def _stage_args(self, parts):
        """int64 words (pointers, weight bits, draws) -> the device copy's
        address, through a pinned buffer that is reused once its copy has left."""
        need = sum(len(p) for p in parts) + 1
        if self._host_args is None or self._host_args.numel() < need:
            self._host_args = torch.empty(need, dtype=torch.int64).pin_memory()
            self._dev_args = torch.empty(need, dtype=torch.int64, device=self.device)
            self._args_done = torch.cuda.Event()
        else:
            self._args_done.synchronize()  # the previous call's copy has left the pinned buffer
        self._host_args.numpy()[:need - 1] = np.concatenate(parts)
        self._dev_args[:need].copy_(self._host_args[:need], non_blocking=True)
        self._args_done.record()
        return self._dev_args.data_ptr()

    def _encode_apply(self, delta, base_arena, payloads, out, wavg):
        """run() from the seeds on: encode, payloads, decode fused with
        apply_delta, the small tensors' float32 payloads and the gap zeroing.
        wavg: (device args, collaborators, weight sum) for the fused encode."""
        dev = self.device
        L = _lib.lib()
        T = len(self.numels)
        fused = wavg is not None
        if fused:
            dp, C, wsum = wavg
        with torch.cuda.device(dev):
            seeds = [int(v) for v in self._seeds[:T].cpu().numpy()] if payloads else None
            # 3. encode, (payloads), decode in place, apply
            result = [None] * len(self.numels) if payloads else None
            if out is None:
                out = self._empty_arena()
            if self.plan is not None:
                p = self.plan
                sd = self._seeds.index_select(0, self._big_idx)
                planes = torch.empty(max(p.planes_bytes, 1), dtype=torch.uint8, device=dev)
                scales = torch.empty(max(p.n_slices, 1), dtype=torch.float32, device=dev)
                if self._codec_ws is None or self._codec_ws.numel() < p.ws_bytes:
                    self._codec_ws = torch.empty(max(p.ws_bytes, 256), dtype=torch.uint8, device=dev)
                if fused:
                    _lib.check(L.ofl_eden_encode_wavg(
                        p.handle, dp, dp + 8 * C, C, wsum, _ptr(base_arena), delta.data_ptr(), sd.data_ptr(),
                        planes.data_ptr(), scales.data_ptr(), self._codec_ws.data_ptr(), self._codec_ws.numel(),
                        _stream(dev)))
                else:
                    p.encode(delta, sd, planes, scales, self._codec_ws)
                if payloads:
                    pn = planes[:p.planes_bytes].cpu().numpy()
                    sn = scales[:p.n_slices].cpu().numpy()
                    for t, i in enumerate(self.big):
                        po, pb, fs = p.planes_offsets[t], p.planes_nbytes[t], p.first_slice[t]
                        md = {0: float(seeds[i]), 1: float(self.numels[i])}
                        for k, (s, d) in enumerate(zip(sn[fs:fs + len(p.dims[t])], p.dims[t])):
                            md[2 + 2 * k] = float(s)
                            md[3 + 2 * k] = float(d)
                        result[i] = (hostmem.bytes_from(pn.ctypes.data + po, pb), [{"int_list": list(self.shapes[i]), "int_to_float": md}])
                if base_arena is not None:  # decode + apply_delta fused: out = base + decoded
                    p.decode(planes, sd, scales, out, self._codec_ws, base=base_arena)
                else:
                    p.decode(planes, sd, scales, delta, self._codec_ws)
            if payloads:
                small = [i for i in range(len(self.numels)) if result[i] is None]
                if small:  # float32 bytes of the delta (Float32NumpyArrayToBytes), one D2H
                    dh = torch.cat([delta[self.offsets[i]:self.offsets[i] + self.numels[i]] for i in small]).cpu().numpy()
                    o = 0
                    for i in small:
                        result[i] = (hostmem.bytes_from(dh.ctypes.data + 4 * o, 4 * self.numels[i]), [{"int_list": list(self.shapes[i])}])
                        o += self.numels[i]
            if base_arena is not None:
                if self.plan is not None:
                    _lib.check_agg(L.ofl_apply_delta_ranges(base_arena.data_ptr(), delta.data_ptr(), out.data_ptr(),
                                                            *self._rest.args, _stream(dev)))
                else:
                    _lib.check_agg(L.ofl_apply_delta(base_arena.data_ptr(), delta.data_ptr(), self.arena_numel,
                                                     out.data_ptr(), _stream(dev)))
            else:
                out.copy_(delta)
            self._zero_gaps(out)
        return out, result, (seeds if payloads else self._seeds[:T])
