"""The Walsh-plane prediction of tests/eden_walsh.py against the C oracle, on
the CPU: what the exact GPU decode checks (tests/test_gpu_eden_decode_designed.py)
stand on.

  * the centroid tables are bitwise antisymmetric for every width;
  * for even p the prediction equals oracle.eden.decompress bit for bit;
  * for odd p the oracle divides by float32(sqrt(P)) twice where the
    prediction (the GPU's documented numerics) multiplies by powers of two:
    three roundings apart (two divisions and the product), 3 * 2^-24 relative
    (1.4e-7 was seen at p = 13);
  * nothing is absorbed: one element moved to a neighbouring bin at P = 2^16
    changes at least 90 % of the oracle's output words;
  * build_batch lays slices, ragged tails and arena gaps where a plan says."""
import types

import numpy as np
import pytest
import torch

from oracle import eden as O
from tests import eden_walsh as W

SCALE = 0.0123


def _ks(bits):
    nv = 1 << bits
    return sorted({0, nv // 2 - 1, nv // 2, nv - 1, (nv // 3) % nv})


def _oracle(P, bits, k, j, seed, scale, bins=None):
    bins = W.walsh_bins(P, bits, k, j) if bins is None else bins
    planes = W.X.expected_planes(bins, [P], bits).numpy()
    return O.decompress(planes, P, [scale], [P], seed, bits)


@pytest.mark.parametrize("bits", range(1, 9))
def test_tables_antisymmetric(bits):
    C, _ = O.tables(bits)
    assert C.dtype == np.float32 and C.size == 1 << bits
    assert np.array_equal(C.view(np.int32), (-C[::-1]).view(np.int32))
    assert np.all(C != 0)


def test_j_set():
    for p in (3, 6, 15, 26):
        js = W.j_set(p)
        P = 1 << p
        assert len(set(js)) == len(js) and all(0 <= j < P for j in js)
        assert {0, 1, P - 1} | {1 << t for t in range(p)} <= set(js)
        assert js == W.j_set(p)


@pytest.mark.parametrize("bits", range(1, 9))
@pytest.mark.parametrize("p", [4, 10, 12, 16])
def test_even_p_equals_oracle_bitwise(p, bits):
    P = 1 << p
    js = W.j_set(p) if p <= 10 else [0, P - 1, 1 << (p - 1), 1 << (p // 2)] + W.j_set(p)[-3:]
    n = 0
    for i, j in enumerate(js):
        for k in (_ks(bits) if i < 3 else _ks(bits)[i % len(_ks(bits)):][:1]):
            seed = (0, 65535, 321, 7)[(i + k) % 4]
            got = W.walsh_expected(P, bits, k, j, seed, SCALE).numpy()
            ref = _oracle(P, bits, k, j, seed, SCALE)
            assert np.array_equal(got.view(np.int32), ref.view(np.int32)), (p, bits, k, j, seed)
            n += 1
    assert n >= 7


@pytest.mark.parametrize("bits", [1, 3, 8])
@pytest.mark.parametrize("p", [5, 11, 13])
def test_odd_p_within_three_roundings(p, bits):
    P = 1 << p
    worst = 0.0
    for i, j in enumerate([0, P - 1, 1 << (p - 1)] + W.j_set(p)[-3:]):
        k = _ks(bits)[i % len(_ks(bits))]
        got = W.walsh_expected(P, bits, k, j, 321 + i, SCALE).numpy().astype(np.float64)
        ref = _oracle(P, bits, k, j, 321 + i, SCALE).astype(np.float64)
        assert np.array_equal(np.signbit(got), np.signbit(ref))
        worst = max(worst, float(np.max(np.abs(got / ref - 1))))
    print(f"[walsh odd p={p} b={bits}] worst relative difference to the oracle {worst:.2e}")
    assert worst <= 3 * 2.0 ** -24


@pytest.mark.parametrize("bits,k", [(8, 255), (8, 128), (3, 4), (1, 0)])
def test_one_moved_bin_changes_nearly_every_word(bits, k):
    p, j, seed = 16, 0x5A5A, 321
    P = 1 << p
    want = W.walsh_expected(P, bits, k, j, seed, SCALE).numpy().view(np.int32)
    bins = W.walsh_bins(P, bits, k, j)
    assert np.array_equal(_oracle(P, bits, k, j, seed, SCALE, bins).view(np.int32), want)
    e = 12345
    b = int(bins[e])
    bins[e] = b - 1 if b > 0 else b + 1
    got = _oracle(P, bits, k, j, seed, SCALE, bins).view(np.int32)
    share = float(np.mean(got != want))
    print(f"[walsh sensitivity b={bits} k={k}] {share:.4f} of the words differ")
    assert share >= 0.90


def test_special_scales_follow_numpy():
    """The expectation for scales no encoder writes is the float32 product
    with the sign pattern: signed zeros, a subnormal, overflow, inf, NaN."""
    P, bits, k, j, seed = 64, 8, 200, 37, 9
    C = O.tables(bits)[0]
    s = W.walsh_expected(P, bits, k, j, seed, 1.0).numpy() / C[k]
    assert set(np.unique(s)) == {-1.0, 1.0}
    for scale in (-0.0123, 0.0, -0.0, 1e-42, np.finfo(np.float32).max, np.inf, np.nan):
        with np.errstate(all="ignore"):
            want = (np.float32(scale) * C[k]) * s
        got = W.walsh_expected(P, bits, k, j, seed, scale).numpy()
        if np.isnan(scale):
            assert np.all(np.isnan(got))
        else:
            assert np.array_equal(got.view(np.int32), want.astype(np.float32).view(np.int32)), scale
            assert np.array_equal(got, _oracle(P, bits, k, j, seed, scale)), scale


def test_build_batch_layout():
    """Two tensors, the second with two slices and a ragged tail (dims
    [65536, 4096], 3000 valid), in a hand-made layout with an arena gap:
    planes, scales and expectation equal the per-tensor oracle decode."""
    bits = 5
    numels = [1024, 68536]
    dims = [[1024], [65536, 4096]]
    plan = types.SimpleNamespace(
        dims=dims, numels=numels, elem_offsets=[0, 1088], arena_numel=1088 + 68536, n_slices=3,
        first_slice=[0, 1], planes_offsets=[0, 640], planes_nbytes=[bits * 128, bits * (65536 + 4096) // 8],
        planes_bytes=640 + bits * (65536 + 4096) // 8)
    specs = [(65535, [(3, 1023, 0.5)]), (0, [(31, 40000, -2.0), (16, 4095, 0.25)])]
    planes, scales, seeds, want, valid = W.build_batch(plan, specs, bits, "cpu")
    assert scales.tolist() == [0.5, -2.0, 0.25] and seeds.tolist() == [65535, 0]
    assert int(valid.sum()) == sum(numels) and not bool(valid[1024:1088].any())
    for t, (seed, runs) in enumerate(specs):
        po, pb = plan.planes_offsets[t], plan.planes_nbytes[t]
        tp = W.tensor_planes(dims[t], bits, runs)
        assert torch.equal(planes[po:po + pb], tp)
        ref = O.decompress(tp.numpy(), numels[t], [r[2] for r in runs], dims[t], seed, bits)
        eo = plan.elem_offsets[t]
        assert np.array_equal(want[eo:eo + numels[t]].numpy(), ref.view(np.int32))
    assert bool((planes[bits * 128:640] == 0xA5).all())
