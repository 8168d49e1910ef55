"""Host side of the lossy round end: lossy.decode_values against the
reference's literal replacement loop (kc_pipeline.py:79-83), and the argument
checks of ofl_kmeans1d_batch_seeds / ofl_label_apply, which return OFL_EINVAL
before any HIP call and so need no device."""
import ctypes

import numpy as np
import pytest


def _reference_backward(int_to_float, nranks):
    """for key in map: data[data == key] = map[key], on a float32 array."""
    data = np.arange(nranks, dtype=np.float32)
    for key in int_to_float:
        data[data == key] = int_to_float[key]
    return data


MAPS = {
    "collision": {0: 2.0, 1: 3.5, 2: 7.0},                       # rank 0 -> 2.0 -> 7.0
    "chain": {0: 1.0, 1: 2.0, 2: 3.0, 3: 0.25},                  # every value is the next key
    "short": {0: -0.5},
    "empty": {},
    "float64": {0: np.float64(-1.2345678901234567e-3), 1: np.float64(0.1), 2: np.float64(1.0) / 3},
    "float32": {i: np.float32(v) for i, v in enumerate([-0.03, -0.01, 0.0, 0.01, 0.02, 0.04])},
    "ternary": {0: np.float64(-1.5e-3), 1: np.float64(0.0), 2: np.float64(1.5e-3)},
    "value_is_own_key": {0: 0.0, 1: 1.0, 2: 5.0},
}


@pytest.mark.parametrize("name", sorted(MAPS))
def test_decode_values_is_the_sequential_replacement(name):
    from openfl_amd import lossy
    m = MAPS[name]
    got = lossy.decode_values(m)
    assert got.dtype == np.float32 and got.shape == (32,)
    np.testing.assert_array_equal(got, _reference_backward(m, 32))
    np.testing.assert_array_equal(lossy.decode_values(m, 8), _reference_backward(m, 8))


def test_decode_values_collision_sends_rank_0_to_the_last_value():
    from openfl_amd import lossy
    got = lossy.decode_values(MAPS["collision"])
    assert got[0] == np.float32(7.0) and got[1] == np.float32(3.5) and got[2] == np.float32(7.0)
    assert got[3] == np.float32(3.0)   # a rank without a key keeps its own value
    # float64 values are rounded to float32 once, as the assignment into a float32 array does
    assert lossy.decode_values(MAPS["float64"])[2] == np.float32(np.float64(1.0) / 3)


def _kmeans_seeds_args(**over):
    """Arguments of ofl_kmeans1d_batch_seeds that pass its checks up to the
    workspace (host arrays only; the device pointers are never followed)."""
    off = np.zeros(1, np.int64)
    num = np.full(1, 100, np.int64)
    seeds = np.ones(1, np.uint64)
    a = {"ntensors": 1, "x": 0x1000, "off": off.ctypes.data, "num": num.ctypes.data, "k": 6, "seeds": seeds.ctypes.data,
         "label": None, "value": None}
    a.update(over)
    keep = (off, num, seeds)
    return keep, (a["ntensors"], a["x"], a["off"], a["num"], a["k"], 6, a["seeds"], 8, 0, None, a["label"], a["value"],
                  None, None, None, None, None, None, 0, None)


@pytest.mark.parametrize("over,msg", [
    ({"seeds": None}, "one seed per tensor"),
    ({"ntensors": 0}, "empty batch"),
    ({"ntensors": -3}, "empty batch"),
    ({"x": None}, "empty batch"),
    ({"off": None}, "empty batch"),
    ({"num": None}, "empty batch"),
    ({"k": 9, "value": 0x2000}, "k <= 8"),
    ({"k": 9, "label": 0x2000}, "k <= 8"),
    ({"k": 0}, "1 <= k <= 32"),
])
def test_kmeans_batch_seeds_refuses_bad_arguments_without_a_device(over, msg):
    from openfl_amd import _lib
    L = _lib.lib()
    keep, args = _kmeans_seeds_args(**over)
    assert L.ofl_kmeans1d_batch_seeds(*args) == _lib.OFL_EINVAL
    assert msg in L.ofl_lossy_last_error().decode()
    del keep


def test_kmeans_batch_seeds_with_good_arguments_gets_as_far_as_the_workspace():
    """The same arguments with nothing wrong are refused only for the missing
    workspace (OFL_ESPACE, still before any HIP call): the cases above fail on
    the argument they name."""
    from openfl_amd import _lib
    L = _lib.lib()
    keep, args = _kmeans_seeds_args()
    assert L.ofl_kmeans1d_batch_seeds(*args) == _lib.OFL_ESPACE
    del keep


@pytest.mark.parametrize("x,recs,n,out", [(None, 0x2000, 1, 0x3000), (0x1000, None, 1, 0x3000),
                                          (0x1000, 0x2000, 1, None), (0x1000, 0x2000, 0, 0x3000),
                                          (0x1000, 0x2000, -1, 0x3000)])
def test_label_apply_refuses_bad_arguments_without_a_device(x, recs, n, out):
    from openfl_amd import _lib
    L = _lib.lib()
    assert L.ofl_label_apply(x, recs, n, None, out, None) == _lib.OFL_EINVAL
    assert "label_apply" in L.ofl_lossy_last_error().decode()


def test_label_record_layout():
    """LabelTable.from_rules writes ofl_label_rec: two int64, eight float32
    midpoints, eight float32 values, 80 bytes."""
    from openfl_amd import lossy
    assert lossy.LabelTable.REC_BYTES == 2 * 8 + 16 * 4
    assert ctypes.sizeof(ctypes.c_int64) == 8
    assert lossy._NEG_TINY < 0 and lossy._NEG_TINY.view(np.uint32) == 0x80000001
