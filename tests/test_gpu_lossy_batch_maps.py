"""The two batched element-wise maps, k_lut_batch (lossy.lut_decode_batch) and
k_ternary_batch (lossy.ternary_ranks_batch), against plain NumPy -- not against
their one-tensor twins:
  LUT      the sequential np.where replacement of lossy.decode_values' rule
           (kc_pipeline.py:79-83), per tensor, in the map's own order;
  ternary  v > 0 -> rank_pos, v < 0 -> rank_neg, else rank_zero.
Results are compared as bit patterns.  One arena per kernel holds the lengths
1, 2, 3, 4, 5, 7, 65535, 65536, 65537 at element offsets = 0, 1, 2, 3 (mod 4):
36 tensors (the block -> tensor search sees T > 32), chunk edges on both sides,
and both branches of the map (16-B accesses where input and output are aligned
together, scalar otherwise); arenas of one and of two tensors are the search's
lo == hi and one-step cases.  Every arena runs with the output aligned like
the input and with the output one element into its buffer (scalar branch
everywhere).  The output is pre-filled with a sentinel: every gap element must
be untouched, and a second run bit-identical.

On an MI355X the module takes 3 s, most of it the host's reference.
"""
import functools

import numpy as np
import pytest
import torch

from tests import topk_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SIZES = (1, 2, 3, 4, 5, 7, C.BLOCK - 1, C.BLOCK, C.BLOCK + 1)
ARENAS = {                                   # name -> [(length, offset mod 4)]
    "all": [(n, mod) for n in SIZES for mod in range(4)],
    "one": [(C.BLOCK + 1, 1)],
    "two": [(5, 3), (C.BLOCK, 0)],
}
MAPS = (
    {},                                                              # empty
    {3: -0.25},                                                      # one key
    {0: -0.031, 1: -0.0, 2: 0.002, 3: 0.25, 4: 1e-40, 5: 7.0},       # six keys (a -0.0 and a denormal value)
    {0: 1.0, 1: 2.0, 2: 7.5, 4: 0.0, 5: 4.0},                        # values equal to later keys: 0 -> 1 -> 2 -> 7.5; 5 -> 4.0 stays
    {j: j + 0.5 for j in range(64)},                                 # 64 keys
)
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x7F800000, 0xFF800000,   # +-0, +-denormal, +-inf
                     0x3FC00000, 0xC0100000, 0x007FFFFF, 0x807FFFFF], np.uint32)               # 1.5, -2.25, largest denormals


@functools.lru_cache(maxsize=None)
def _layout(name):
    sizes = [n for n, _ in ARENAS[name]]
    a, offs, gap = C.arena([np.zeros(n, np.float32) for n in sizes], [m for _, m in ARENAS[name]])
    assert [o % 4 for o in offs] == [m for _, m in ARENAS[name]] and a.size < 1_000_000
    gap.setflags(write=False)
    return a.size, offs, sizes, gap


@functools.lru_cache(maxsize=None)
def _lut_case(name, rot):
    """Ranks 0..5 in every tensor, tensor t under MAPS[(t + rot) % 5] -> (input, maps, expected bits)."""
    size, offs, sizes, _ = _layout(name)
    rng = np.random.default_rng(1000 + rot)
    x = np.zeros(size, np.float32)
    want = np.zeros(size, np.float32)
    maps = []
    for t, (o, n) in enumerate(zip(offs, sizes)):
        m = MAPS[(t + rot) % len(MAPS)]
        v = rng.integers(0, 6, n).astype(np.float32)
        x[o:o + n] = v
        for key, val in m.items():                                   # in place and in sequence, as the reference
            v = np.where(v == np.float32(key), np.float32(val), v)
        want[o:o + n] = v
        maps.append(m)
    for a in (x, want):
        a.setflags(write=False)
    return x, maps, want.view(np.uint32)


@functools.lru_cache(maxsize=None)
def _ternary_case(name):
    size, offs, sizes, _ = _layout(name)
    rng = np.random.default_rng(7)
    x = np.zeros(size, np.uint32)
    want = np.zeros(size, np.float32)
    ranks3 = np.array([[3 * t + 0.5, 3 * t + 1.5, 3 * t + 2.5] for t in range(len(sizes))], np.float32)   # distinct per tensor
    for t, (o, n) in enumerate(zip(offs, sizes)):
        bits = SPECIALS[rng.integers(0, SPECIALS.size, n)]
        bits[:min(n, SPECIALS.size)] = SPECIALS[:min(n, SPECIALS.size)]   # every special in every tensor that has room
        x[o:o + n] = bits
        v = bits.view(np.float32)
        rn, rz, rp = ranks3[t]
        want[o:o + n] = np.where(v > 0, rp, np.where(v < 0, rn, rz))
    x = x.view(np.float32)
    for a in (x, want, ranks3):
        a.setflags(write=False)
    return x, ranks3, want.view(np.uint32)


def _check(name, shifted, x, want, run):
    """run(x_dev, out_dev) twice into a sentinel-filled output (a view one
    element into its buffer if shifted): tensors bit-exact, gaps untouched,
    second run identical."""
    size, offs, sizes, gap = _layout(name)
    x_dev = torch.from_numpy(x.copy()).to(DEV)
    assert x_dev.data_ptr() % 16 == 0
    outs = []
    for _ in range(2):
        buf = torch.from_numpy(np.full(size + 1, C.SENTINEL, np.uint32).view(np.float32)).to(DEV)
        out = buf[1:] if shifted else buf[:size]
        assert out.data_ptr() % 16 == (4 if shifted else 0)
        run(x_dev, out)
        got = buf.cpu().numpy().view(np.uint32)
        assert got[0 if shifted else size] == C.SENTINEL               # the element of the buffer outside the view
        outs.append(got[1:] if shifted else got[:size])
    np.testing.assert_array_equal(outs[0], outs[1])
    assert np.all(outs[0][gap] == C.SENTINEL), int(np.sum(outs[0][gap] != C.SENTINEL))
    bad = [(t, n, o % 4, int(np.sum(outs[0][o:o + n] != want[o:o + n])))
           for t, (o, n) in enumerate(zip(offs, sizes)) if not np.array_equal(outs[0][o:o + n], want[o:o + n])]
    assert not bad, bad[:20]


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "out_plus_1"])
@pytest.mark.parametrize("name,rot", [("all", r) for r in range(len(MAPS))] + [("one", 2), ("one", 4), ("two", 3)])
def test_lut_batch_is_the_sequential_replacement(name, rot, shifted):
    from openfl_amd import lossy
    x, maps, want = _lut_case(name, rot)
    _, offs, sizes, _ = _layout(name)
    _check(name, shifted, x, want, lambda xd, od: lossy.lut_decode_batch(xd, offs, sizes, maps, od))


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "out_plus_1"])
@pytest.mark.parametrize("name", list(ARENAS))
def test_ternary_batch_is_the_sign_rule(name, shifted):
    from openfl_amd import lossy
    x, ranks3, want = _ternary_case(name)
    _, offs, sizes, _ = _layout(name)
    _check(name, shifted, x, want, lambda xd, od: lossy.ternary_ranks_batch(xd, offs, sizes, ranks3, od))


def test_the_cases_are_the_designed_ones():
    """The reference itself: the chain map chains, -0.0 and the denormals land
    on the sign rule's sides, every map meets every tensor of the big arena."""
    dec = np.arange(6, dtype=np.float32)
    for key, val in MAPS[3].items():
        dec = np.where(dec == np.float32(key), np.float32(val), dec)
    assert dec.tolist() == [7.5, 7.5, 7.5, 3.0, 0.0, 4.0]
    v = SPECIALS.view(np.float32)
    assert np.where(v > 0, 2, np.where(v < 0, 0, 1)).tolist() == [1, 1, 2, 0, 2, 0, 2, 0, 2, 0]
    assert [len(m) for m in MAPS] == [0, 1, 6, 5, 64]
    assert len(ARENAS["all"]) == 36 and len(MAPS) == 5     # t + rot over all rotations: every (tensor, map) pair
