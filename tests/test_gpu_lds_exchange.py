"""Bit-identity of the row passes across the change of their LDS exchange:
planes, scales and decoded values of small large-slice plans against digests
recorded with the library built from the commit before the lane-linear
exchange (tests/golden/lds_exchange_parent.json; `python -m
tests.test_gpu_lds_exchange OUT.json` records them with whatever library
OFL_CODEC_LIB names).  Only the LDS image between two register layouts
changed, so every output bit must stay."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lds_exchange_parent.json")
N_BITS = (1, 4, 8)
# 2^16: two row tiles, the smallest large slice; 2^18: the smallest with tile
# pairs; 2^21 - 99,997: a ragged last tile; 2^22 x 8 in one plan: a full wave,
# the tile-table path.  (k_col6 keeps its exchange, so no five-pass slice.)
SHAPES = {
    "2^16": [1 << 16],
    "2^18": [1 << 18],
    "2^21-99997": [(1 << 21) - 99_997],
    "2^22x8": [1 << 22] * 8,
}
# the library's default plan, and the two-blocks-per-CU row kernels forced
# (k_enc_rowA2, k_enc_rowC2, k_dec_rowA2, k_dec_rowC2): bit-identical plans
ROW2 = (None, 1)


def _inputs(numels):
    """Seeded N(0, 0.01^2) from the CPU generator, one draw per tensor."""
    g = torch.Generator().manual_seed(20_261 + len(numels) + numels[0] % 1000)
    return [torch.empty(n, dtype=torch.float32).normal_(0, 0.01, generator=g) for n in numels]


def _sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def compute():
    """{shape: {n_bits: {row2: {planes, y, scales}}}} with the loaded library."""
    from openfl_amd.codec import EdenPlan
    dev = torch.device("cuda")
    out = {}
    for name, numels in SHAPES.items():
        xs = _inputs(numels)
        seeds = torch.arange(11, 11 + len(numels), dtype=torch.int32, device=dev)
        out[name] = {}
        for nb in N_BITS:
            out[name][str(nb)] = {}
            for row2 in ROW2:
                plan = EdenPlan(numels, nb) if row2 is None else EdenPlan(numels, nb, row2=row2)
                x = torch.zeros(plan.arena_numel, device=dev)
                for o, t in zip(plan.elem_offsets, xs):
                    x[o:o + t.numel()] = t.to(dev)
                ws = torch.empty(max(plan.ws_bytes, 256), dtype=torch.uint8, device=dev)
                p = torch.full((plan.planes_bytes,), 0x5A, dtype=torch.uint8, device=dev)
                s = torch.full((plan.n_slices,), float("nan"), dtype=torch.float32, device=dev)
                y = torch.full((plan.arena_numel,), float("nan"), dtype=torch.float32, device=dev)
                plan.encode(x, seeds, p, s, ws)
                plan.decode(p, seeds, s, y, ws)
                torch.cuda.synchronize()
                names = sorted({l["name"].split("::")[-1].split("<")[0] for e in (True, False) for l in plan.launches(e)})
                out[name][str(nb)]["default" if row2 is None else "row2"] = {
                    "planes": _sha([p[o:o + b] for o, b in zip(plan.planes_offsets, plan.planes_nbytes)]),
                    "y": _sha([y[o:o + n] for o, n in zip(plan.elem_offsets, plan.numels)]),
                    "scales": [int(v) for v in s[:plan.n_slices].cpu().numpy().view(np.uint32)],
                    "kernels": names,
                }
    return out


@pytest.fixture(scope="module")
def head():
    return compute()


@pytest.fixture(scope="module")
def parent():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_outputs_equal_the_parent_build(head, parent, shape):
    """SHA-256 of the planes and of the decoded values, and the raw scale
    words, equal the parent build's at n_bits 1, 4 and 8, on the default plan
    and with the two-block row kernels forced."""
    assert set(parent[shape]) == {str(b) for b in N_BITS}
    for nb in N_BITS:
        for cfg in ("default", "row2"):
            got, want = head[shape][str(nb)][cfg], parent[shape][str(nb)][cfg]
            assert all(np.isfinite(np.array(want["scales"], dtype=np.uint32).view(np.float32))), (shape, nb, cfg)
            for key in ("scales", "planes", "y"):
                assert got[key] == want[key], (shape, nb, cfg, key)


def test_the_converted_kernels_ran(head):
    """The plans above launch the kernels whose exchange changed."""
    ran = set()
    for per_shape in head.values():
        for per_nb in per_shape.values():
            ran |= set(per_nb["row2"]["kernels"])
    assert {"k_enc_rowA2", "k_enc_rowC2", "k_dec_rowA2", "k_dec_rowC2"} <= ran, ran


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(compute(), f, indent=1, sort_keys=True)
        f.write("\n")
