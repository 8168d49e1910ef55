"""CPU checks of the designed-input machinery (tests/eden_exact.py): the
designed bins are the reference's own (hash of its planes, recorded in
tests/golden/eden_designed.json by make_golden.py --only designed), the torch
FWHT is the oracle's, and the oracle encodes / decodes the designed inputs
exactly.  The GPU kernels meet the same inputs in tests/test_gpu_eden_exact.py."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import eden as O
from tests import eden_exact as X
from tests.golden_io import GOLDEN

with open(os.path.join(GOLDEN, "eden_designed.json")) as _f:
    CASES = json.load(_f)["cases"]
_built = {}


def _case(case):
    """designed() of a fixture case, built once and shared (never modified)."""
    key = (tuple(case["dims"]), case["bits"])
    if key not in _built:
        assert case["seed"] == X.SEED and case["rng_seed"] == [X.SEED, case["bits"]] + case["dims"]
        x, bins, alphas = X.designed(case["dims"], case["bits"])
        assert alphas == case["alphas"]
        _built[key] = (x.numpy(), bins, alphas)
    return _built[key]


def _id(case):
    return f"b{case['bits']}_" + "_".join(str(d) for d in case["dims"])


def test_fixture_covers_the_cases():
    assert [(c["dims"], c["bits"]) for c in CASES] == [(d, b) for d in X.FIXTURE_DIMS for b in range(1, 9)]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_designed_bins_are_the_references(case):
    """sha256(expected_planes(designed bins)) is the hash of the planes the
    reference's Eden.compress wrote for this input: the designed bins are the
    reference's answer, not the oracle's or ours.  Its scales are held only to
    its own accuracy (a sequential fp32 norm: up to 1.9e-3 off at 2^20)."""
    _, bins, alphas = _case(case)
    planes = X.expected_planes(bins, case["dims"], case["bits"]).numpy()
    assert planes.size == case["planes_len"]
    assert hashlib.sha256(planes.tobytes()).hexdigest() == case["planes_sha256"]
    np.testing.assert_allclose(case["scales"], alphas, rtol=3e-3)
    # every bin value is there where the slice has room for it
    off = 0
    for P in case["dims"]:
        if P >= 4 << case["bits"]:
            assert len(torch.unique(bins[off:off + P])) == 1 << case["bits"]
        off += P


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_oracle_encodes_designed_exactly(case):
    """oracle.eden.compress returns exactly the designed bins and
    |scale / alpha - 1| <= 1e-6 (fp32 rotation noise ~1e-6 against a margin
    of >= 2e-3; its sums run in double: measured <= 2.1e-7)."""
    x, bins, alphas = _case(case)
    planes, scales, dims, total = O.compress(x, X.SEED, case["bits"])
    assert dims == case["dims"] and total == sum(dims)
    got = O.bins_of(planes, sum(dims), case["bits"])
    assert np.array_equal(got, bins.numpy()), int(np.count_nonzero(got != bins.numpy()))
    assert np.array_equal(planes, X.expected_planes(bins, dims, case["bits"]).numpy())
    worst = max(abs(s / a - 1) for s, a in zip(scales, alphas))
    assert worst <= 1e-6, worst


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_oracle_decodes_designed_planes_to_x(case):
    """oracle.eden.decompress(expected planes, scale = alpha) is x within
    relative L2 1e-6 (measured 2.1e-7 to 3.2e-7)."""
    x, bins, alphas = _case(case)
    dims = case["dims"]
    planes = X.expected_planes(bins, dims, case["bits"]).numpy()
    y = O.decompress(planes, sum(dims), alphas, dims, X.SEED, case["bits"])
    rel = np.linalg.norm(y.astype(np.float64) - x) / np.linalg.norm(x.astype(np.float64))
    assert rel <= 1e-6, rel


@pytest.mark.parametrize("P", [1 << 11, 1 << 16])
def test_torch_fwht_is_the_oracles(P):
    """eden_exact.fwht against oracle.eden.fwht, in fp32 and in fp64, within
    1e-6 of the largest value; rotate / unrotate are inverses and use
    rand_diag's signs."""
    v = np.random.default_rng(P).standard_normal(P).astype(np.float32)
    ref = O.fwht(v).astype(np.float64)
    bar = 1e-6 * np.max(np.abs(ref))
    for dt in (torch.float32, torch.float64):
        got = X.fwht(torch.from_numpy(v).to(dt)).double().numpy()
        assert np.max(np.abs(got - ref)) <= bar, dt
    assert np.array_equal(X.signs(P, 7, torch.float32, "cpu").numpy(), O.rand_diag(P, 7))
    t = torch.from_numpy(v).double()
    want = O.fwht(O.fwht(v * O.rand_diag(P, 7)) * O.rand_diag(P, 8)).astype(np.float64)
    assert np.max(np.abs(X.rotate(t, 7).numpy() - want)) <= 1e-6 * np.max(np.abs(want))
    assert float((X.unrotate(X.rotate(t, 7), 7) - t).abs().max()) <= 1e-12


def test_small_slices_and_tiny_dims_build():
    """Slices below 4 * 2^bits (no room to force every value) still meet the
    margin, with distinct values where the draw allows."""
    for dims in ([8], [64], [1024], [1 << 15]):
        for bits in range(1, 9):
            x, bins, _ = X.designed(dims, bits)
            planes, scales, _, _ = O.compress(x.numpy(), X.SEED, bits)
            assert np.array_equal(O.bins_of(planes, dims[0], bits), bins.numpy()), (dims, bits)
            assert abs(scales[0] / 0.01 - 1) <= 1e-6


def test_margin_assertion_fires_on_skewed_bins():
    """Four of every value forced into one 2^16 slice at 8 bits, not
    rebalanced: rms(C[bins]) moves by 1.5 %, the outer centroids leave their
    cells (29 685 bins moved in the reference), and the builder must refuse."""
    with pytest.raises(AssertionError, match="margin"):
        X.designed([1 << 16], 8, force_each=4, rebalance=False)
    X.designed([1 << 16], 8, force_each=4)  # rebalanced, the same recipe holds


def test_margin_rule_accepts_the_oracle_and_rejects_a_shifted_bin():
    """margin_rule on a ragged slice: the oracle's own bins pass, with the
    excluded share under 1e-3; one bin moved by two fails wherever it lies."""
    n, bits = 120_003, 8
    x = np.random.default_rng(3).standard_normal(n).astype(np.float32) * np.float32(0.01)
    planes, _, dims, _ = O.compress(x, X.SEED, bits)
    got = torch.from_numpy(O.bins_of(planes, sum(dims), bits).astype(np.int32))
    xt = torch.from_numpy(x)
    share = X.margin_rule(xt, n, dims, bits, X.SEED, got)
    assert share <= 1e-3, share
    bad = got.clone()
    bad[5] += 2 if bad[5] < 254 else -2
    with pytest.raises(AssertionError):
        X.margin_rule(xt, n, dims, bits, X.SEED, bad)
