"""Host side of the streaming round end: the two new entry points are declared,
exported and bound, refuse bad arguments before any HIP call, and without a
device accumulator() / ingest() / finish() raise CodecError like every other
call of the package (no CPU fallback)."""
import re

import pytest

from tests import golden_io

NEW = ("ofl_wavg_accumulate", "ofl_wavg_finish")


def test_new_symbols_are_declared_exported_and_bound():
    import ctypes

    from openfl_amd import _lib
    L = _lib.lib()
    with open(f"{golden_io.GOLDEN}/../../include/ofl_codec.h") as f:
        declared = set(re.findall(r"\b(ofl_[a-z0-9_]+)\s*\(", f.read()))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).restype is ctypes.c_int
    assert L.ofl_wavg_accumulate.argtypes == [ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_int64,
                                              ctypes.c_void_p, ctypes.c_void_p]
    assert L.ofl_wavg_finish.argtypes == [ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_int64,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]


@pytest.mark.parametrize("call,args", [
    ("ofl_wavg_accumulate", (None, 1.0, 1, 4, 0x2000, None)),
    ("ofl_wavg_accumulate", (0x1000, 1.0, 1, 4, None, None)),
    ("ofl_wavg_accumulate", (0x1000, 1.0, 0, -1, 0x2000, None)),
    ("ofl_wavg_finish", (None, 1.0, None, 4, None, None, None)),
    ("ofl_wavg_finish", (0x1000, 1.0, None, -1, None, None, None)),
    ("ofl_wavg_finish", (0x1000, 1.0, None, 4, 0x1000, None, None)),
])
def test_bad_arguments_are_refused_without_a_device(call, args):
    from openfl_amd import _lib
    L = _lib.lib()
    assert getattr(L, call)(*args) == _lib.OFL_EINVAL
    assert call[4:] in L.ofl_agg_last_error().decode()


def test_empty_arenas_are_no_work():
    from openfl_amd import _lib
    L = _lib.lib()
    assert L.ofl_wavg_accumulate(None, 1.0, 1, 0, None, None) == _lib.OFL_OK
    assert L.ofl_wavg_finish(None, 1.0, None, 0, None, None, None) == _lib.OFL_OK


def test_without_a_device_every_new_call_raises(monkeypatch):
    import torch

    from openfl_amd._lib import CodecError
    from openfl_amd.aggregation import RoundEnd, WavgAccumulator
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(CodecError, match="GPU"):
        from openfl_amd.pipelines import EdenPipeline
        RoundEnd(EdenPipeline(), [(4,)])
    re_ = object.__new__(RoundEnd)   # as far as a RoundEnd gets without a device
    with pytest.raises(CodecError, match="GPU"):
        re_.accumulator()
    with pytest.raises(CodecError, match="GPU"):
        re_.ingest([])
    with pytest.raises(CodecError, match="GPU"):
        re_.finish(WavgAccumulator(re_, None))
