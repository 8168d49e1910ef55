"""GPU: RoundEnd.ingest, one collaborator's upload into a device arena.

The uploads are made with the project's own pipelines' forward per tensor and
the yardstick is their own per-tensor backward (+ the base in float32), which
the golden tests pin to the reference: arena bits per tensor, zero gaps.  The
same upload in three metadata forms (dicts, float32-rounded values, the
protobuf containers), uploads made of the reference's own payload bytes
(tests/golden), the > / >= threshold case, and the checks, each of which
leaves `out` untouched."""
import copy
import functools
import gzip

import numpy as np
import pytest
import torch

from tests import golden_io
from tests.round_stream_cases import (DEV, DIM_THRESHOLD, F, SHAPES, SHAPES_ROW, bits, gap_mask, make_pipeline, md_key,
                                      shapes_for, tensors)

pytestmark = pytest.mark.gpu
SENTINEL = 123.25
KINDS = ("eden_fast", "kc", "skc", "stc")


@functools.lru_cache(maxsize=None)
def _round_end(name, shapes=tuple(SHAPES)):
    from openfl_amd.aggregation import RoundEnd
    return RoundEnd(make_pipeline(name), list(shapes), device=DEV)


@functools.lru_cache(maxsize=None)
def _upload(name, lossless, shapes=tuple(SHAPES)):
    """(the pipeline that decodes it, [(payload, metadata list)] per tensor);
    shared, never modified."""
    from openfl_amd.pipelines import NoCompressionPipeline
    pipe = NoCompressionPipeline() if lossless else _round_end(name, shapes).pipeline
    np.random.seed(11)
    return pipe, [pipe.forward(x) for x in tensors(shapes, 21)]


def _backward(pipe, items):
    """The yardstick: the pipeline's own backward per tensor (on copies of the
    metadata lists, which it pops)."""
    return [np.asarray(pipe.backward(p, list(mds)), F) for p, mds in items]


def _check(re, arena, want):
    got = arena.cpu().numpy()
    assert got.size == re.arena_numel
    for i, y in enumerate(want):
        o, n = re.offsets[i], re.numels[i]
        assert y.shape == re.shapes[i], i
        assert bits(got[o:o + n]) == bits(y.reshape(-1)), i
    assert not got[gap_mask(re)].view(np.uint32).any()


@pytest.mark.parametrize("delta", [True, False], ids=["delta", "nodelta"])
@pytest.mark.parametrize("lossless", [True, False], ids=["lossless", "lossy"])
@pytest.mark.parametrize("name", KINDS)
def test_ingest_equals_backward(name, lossless, delta):
    shapes = shapes_for(name)
    re = _round_end(name, shapes)
    pipe, items = _upload(name, lossless, shapes)
    base_h = tensors(shapes, 3, 0.1)
    base = re.pack(base_h)
    want = _backward(pipe, items)
    if delta:
        want = [b + y for b, y in zip(base_h, want)]
    got = re.ingest(items, lossless=lossless, delta=delta, base_arena=base if delta else None)
    _check(re, got, want)
    assert bits(base.cpu().numpy()) == bits(re.pack(base_h).cpu().numpy())
    # into a given arena, whatever it held
    out = torch.full((re.arena_numel,), SENTINEL, dtype=torch.float32, device=DEV)
    assert re.ingest(items, lossless=lossless, delta=delta, base_arena=base if delta else None, out=out) is out
    _check(re, out, want)
    if delta:   # the base's own arena
        assert re.ingest(items, lossless=lossless, delta=True, base_arena=base, out=base) is base
        _check(re, base, want)


@pytest.mark.parametrize("delta", [True, False], ids=["delta", "nodelta"])
def test_ingest_with_a_row_pass_slice(delta):
    re = _round_end("eden_fast", tuple(SHAPES_ROW))
    assert any(P > 1 << 15 for d in re.plan.dims for P in d)
    pipe, items = _upload("eden_fast", False, tuple(SHAPES_ROW))
    base_h = tensors(SHAPES_ROW, 3, 0.1)
    want = _backward(pipe, items)
    if delta:
        want = [b + y for b, y in zip(base_h, want)]
    _check(re, re.ingest(items, delta=delta, base_arena=re.pack(base_h) if delta else None), want)


def _rounded(items):
    """What the wire gives: int_to_float values rounded to float32."""
    out = []
    for p, mds in items:
        new = []
        for md in mds:
            md = dict(md)
            if md.get("int_to_float") is not None:
                md["int_to_float"] = {k: float(F(v)) for k, v in md["int_to_float"].items()}
            new.append(md)
        out.append((p, new))
    return out


def _through_protobuf(items):
    from openfl_amd import protocols as P
    out = []
    for i, (p, mds) in enumerate(items):
        nt = P.construct_named_tensor((f"t{i}", "col", 0, False, ("trained",)), p, mds, False)
        back = P.NamedTensor()
        back.ParseFromString(nt.SerializeToString())
        out.append((back.data_bytes, P.transformer_metadata_of(back)))
    return out


def _snapshot(items):
    return [(p, len(mds), md_key([{k: v for k, v in md.items() if k != "bool_list" and len(v)} for md in mds]))
            for p, mds in items]


@pytest.mark.parametrize("name", ["eden_fast", "skc"])
def test_three_metadata_forms(name):
    re = _round_end(name, shapes_for(name))
    pipe, items = _upload(name, False, shapes_for(name))
    forms = {"dicts": copy.deepcopy(items), "rounded": _rounded(items), "protobuf": _through_protobuf(items)}
    got = {}
    for form, its in forms.items():
        before = _snapshot(its)
        got[form] = re.ingest(its, delta=False)
        assert _snapshot(its) == before, form        # items are left as they were
        _check(re, got[form], _backward(pipe, its))   # backward on that same metadata
        assert _snapshot(its) == before, form
    assert bits(got["rounded"].cpu().numpy()) == bits(got["protobuf"].cpu().numpy())


def test_threshold_is_greater_than():
    """100 elements (== dim_threshold) travel raw, 101 as Eden planes."""
    re = _round_end("eden_fast")
    _, items = _upload("eden_fast", False)
    i100, i101 = SHAPES.index((10, 10)), SHAPES.index((101,))
    assert DIM_THRESHOLD == 100 and len(items[i100][0]) == 400 and "int_to_float" not in items[i100][1][0]
    assert len(items[i101][0]) == 104 and items[i101][1][0]["int_to_float"][1] == 101.0
    assert i100 not in re.big and i101 in re.big


def _assert_decode_close(y, ref):
    """tests/test_gpu_parity.py's bound for the decode of reference planes."""
    ref, y = ref.astype(np.float64), y.astype(np.float64)
    assert np.max(np.abs(y - ref)) <= 2e-6 * max(np.max(np.abs(ref)), 1e-30)
    assert np.linalg.norm(y - ref) <= 2e-6 * np.linalg.norm(ref)


def test_upload_of_the_references_eden_payloads():
    from openfl_amd.aggregation import RoundEnd
    arr, idx = golden_io.eden()
    cases = {c["tag"]: c for c in idx["eden_cases"]}
    cases = [cases[t] for t in ("b8_n101", "b8_n100", "b8_n1000", "b8_n37000", "b8_n65537")]
    items = []
    for c in cases:
        if c["n"] > DIM_THRESHOLD:
            items.append((arr[c["planes_key"]].tobytes(), [{"int_list": [c["n"]], "int_to_float": golden_io.metadata_of(c)}]))
        else:   # the reference sends it raw
            items.append((arr[c["y_key"]].tobytes(), [{"int_list": [c["n"]]}]))
    re = RoundEnd(make_pipeline("eden_fast"), [(c["n"],) for c in cases], device=DEV)
    got = re.ingest(items, delta=False).cpu().numpy()
    for i, c in enumerate(cases):
        _assert_decode_close(got[re.offsets[i]:re.offsets[i] + c["n"]], arr[c["y_key"]])
    assert not got[gap_mask(re)].any()


def test_upload_of_the_references_kc_streams():
    """gzip.compress streams (no member index: the inflate's host fallback)
    and the reference's maps; n = 5 goes the pipeline's host path."""
    from openfl_amd.aggregation import RoundEnd
    arr, idx = golden_io.lossy()
    items = []
    for rec in idx["kc"]:
        n = rec["n"]
        md = {"int_list": rec["int_list"], "int_to_float": {int(k): v for k, v in rec["int_to_float"]}}
        items.append((gzip.compress(arr[f"kcint_n{n}"].astype(F).tobytes()), [md, {}]))
    re = RoundEnd(make_pipeline("kc"), [tuple(rec["int_list"]) for rec in idx["kc"]], device=DEV)
    got = re.ingest(items, delta=False).cpu().numpy()
    for i, rec in enumerate(idx["kc"]):
        want = arr[f"kcy_n{rec['n']}"]
        np.testing.assert_array_equal(got[re.offsets[i]:re.offsets[i] + want.size], want.reshape(-1))


def _bad_uploads(name, items):
    """(what is wrong, the items, the message) per check of ingest."""
    i101 = SHAPES.index((101,))
    cut = lambda i, k: [(p[:k], m) if j == i else (p, m) for j, (p, m) in enumerate(items)]  # noqa: E731
    bad = [("count", items[:-1], "items"),
           ("int_list", [(p, [dict(m[0], int_list=[7, 1])] + list(m[1:])) if j == 2 else (p, m)
                         for j, (p, m) in enumerate(items)], "tensor 2: int_list")]
    if name == "lossless":
        bad.append(("short", cut(6, 4 * 40000 - 4), "tensor 6: payload has"))
    elif name == "eden_fast":
        bad.append(("short planes", cut(i101, 103), f"tensor {i101}: payload has 103"))
        bad.append(("short raw", cut(2, 27), "tensor 2: payload has 27"))
        m = dict(items[i101][1][0]["int_to_float"])
        m[1] = 100.0
        foreign = [(p, [dict(md[0], int_to_float=m)]) if j == i101 else (p, md) for j, (p, md) in enumerate(items)]
        bad.append(("slice plan", foreign, f"tensor {i101}: Eden metadata"))
    else:
        bad.append(("short", cut(6, 10), "tensor 6: payload has 10"))
    return bad


@pytest.mark.parametrize("name", ["lossless", "eden_fast", "kc"])
def test_checks_leave_out_untouched(name):
    from openfl_amd._lib import CodecError
    re = _round_end("eden_fast" if name == "lossless" else name)
    _, items = _upload("eden_fast", True) if name == "lossless" else _upload(name, False)
    base = re.pack(tensors(SHAPES, 3, 0.1))
    out = torch.full((re.arena_numel,), SENTINEL, dtype=torch.float32, device=DEV)
    kw = {"lossless": name == "lossless"}
    with pytest.raises(CodecError, match="needs base_arena"):
        re.ingest(items, delta=True, out=out, **kw)
    for what, its, msg in _bad_uploads(name, items):
        for delta in (True, False):
            with pytest.raises(CodecError, match=msg):
                re.ingest(its, delta=delta, base_arena=base if delta else None, out=out, **kw)
            assert (out == SENTINEL).all(), (what, delta)
    with pytest.raises(CodecError, match="arenas must be"):
        re.ingest(items, delta=False, out=out[:re.arena_numel - 1], **kw)
    # and the good upload still decodes after all that
    re.ingest(items, delta=False, out=out, **kw)
    assert not (out == SENTINEL).any()
