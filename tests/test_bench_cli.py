"""bench.py's command line: a plain run reports the timed steps only, --full
keeps the rest, --dump-outputs writes the last timed step's outputs."""
import json
import os

import numpy as np
import pytest

import bench


def test_plain_is_the_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_full_only_options_are_named():
    a = bench.parse_args(["--steps", "3", "--also", "", "--traffic-json", "t.json", "--streams", "1"])
    assert bench.full_only_given(a) == ["--also", "--traffic-json"]
    assert bench.full_only_given(bench.parse_args(["--steps", "3", "--dump-outputs", "d"])) == []


def test_sample_positions():
    segs = [(0, 10), (64, 0), (128, 5), (1000, 100_000)]
    every = bench._sample_positions(segs, 1 << 20, 1)          # fewer than k: all of them, in order
    want = np.concatenate([np.arange(o, o + n) for o, n in segs])
    np.testing.assert_array_equal(every, want)
    some = bench._sample_positions(segs, 5000, 1)
    assert some.dtype == np.int64 and some.shape == (5000,) and np.all(np.diff(some) >= 0)
    assert np.all(np.isin(some, want))                          # never in the padding between segments
    assert some[0] < 1000 <= some[-1]                           # reaches across segments
    np.testing.assert_array_equal(some, bench._sample_positions(segs, 5000, 1))
    assert not np.array_equal(some, bench._sample_positions(segs, 5000, 2))
    assert bench._sample_positions([], 16, 1).size == 0
    big = bench._sample_positions([(0, 1 << 33), (1 << 34, 1 << 33)], 1000, 3)   # positions past 2^31
    assert big.max() >= 1 << 34 and big.max() < (1 << 34) + (1 << 33)
    assert not np.any((big >= 1 << 33) & (big < 1 << 34))


def _run(capsys, *argv):
    assert bench.main(list(argv)) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_and_dump(tmp_path, capsys):
    """mnist_cnn (8 tensors, 431,080 elements: every element is dumped).  The
    line has the timed figure and none of the --full extras; y is the decode
    of the seeded input (8-bit Eden: about 6e-3 relative L2, DESIGN.md
    section 4; 2e-2 bounds it); a second run writes the same bytes."""
    import torch
    from openfl_amd.workloads import WORKLOADS, numel
    args = ["--gpus", "1", "--workload", "mnist_cnn", "--steps", "2", "--warmup", "1"]
    d = _run(capsys, *args, "--dump-outputs", str(tmp_path / "a"))
    assert d["steps"] == 2 and d["warmup"] == 1 and d["full"] is False
    assert d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "GiB/s" and d["higher_is_better"] is True
    assert d["also"] is None and d["cpu_baseline"] is None and d["check_rel_l2"] is None
    assert "kernels" not in d["roofline"] and d["roofline"]["traffic"] is None
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("y", "planes", "scales")}
    assert sorted(os.listdir(tmp_path / "a")) == ["planes.npy", "scales.npy", "y.npy"]
    assert all(a.dtype == np.float32 and a.ndim == 1 for a in got.values())
    numels = [numel(s) for _, s in WORKLOADS["mnist_cnn"]()]
    assert got["y"].size == sum(numels) and got["scales"].size == d["config"]["slices_rank0"]
    assert 0 < got["planes"].size <= d["config"]["planes_bytes_rank0"]
    assert np.all(got["planes"] == np.floor(got["planes"])) and got["planes"].min() >= 0 and got["planes"].max() <= 255
    gen = torch.Generator(device="cuda:0")
    xs = []
    for i, n in enumerate(numels):
        gen.manual_seed(i)
        xs.append(torch.empty(n, dtype=torch.float32, device="cuda:0").normal_(0.0, 0.01, generator=gen).cpu().numpy())
    x = np.concatenate(xs).astype(np.float64)
    rel = np.linalg.norm(got["y"] - x) / np.linalg.norm(x)
    print(f"rel L2 of the dumped y against x: {rel:.3e}")
    assert rel < 2e-2
    # the three files belong together: the oracle's decode of each tensor's
    # dumped planes and scales (the plan's layout, bench.py's seeds) is the
    # dumped y, within the bound the HIP decoder is held to against the
    # oracle's decode of the same bytes (test_gpu_e2e.py: 2e-6 x max |ref|)
    from oracle import eden as O
    from openfl_amd.codec import EdenPlan
    plan = EdenPlan(numels, 8)
    assert got["planes"].size == sum(plan.planes_nbytes)
    seeds = np.random.RandomState(1234).randint(0, 2 ** 16, size=len(numels))
    planes_u8 = got["planes"].astype(np.uint8)
    po = eo = 0
    for t, n in enumerate(numels):
        sc = got["scales"][plan.first_slice[t]:plan.first_slice[t] + len(plan.dims[t])]
        ref = O.decompress(planes_u8[po:po + plan.planes_nbytes[t]], n, sc, plan.dims[t], int(seeds[t]), 8)
        err = np.max(np.abs(got["y"][eo:eo + n].astype(np.float64) - ref))
        print(f"tensor {t}: max |y - oracle decode| {err:.3e}, max |ref| {np.max(np.abs(ref)):.3e}")
        assert err <= 2e-6 * max(np.max(np.abs(ref)), 1e-30)
        po += plan.planes_nbytes[t]
        eo += n
    _run(capsys, *args, "--dump-outputs", str(tmp_path / "b"))
    for n, a in got.items():
        assert a.tobytes() == np.load(tmp_path / "b" / f"{n}.npy").tobytes(), n


@pytest.mark.gpu
def test_full_keeps_the_extras(capsys):
    d = _run(capsys, "--gpus", "1", "--workload", "mnist_cnn", "--steps", "2", "--warmup", "1", "--full",
             "--also", "", "--cpu-budget-s", "0.2")
    assert d["full"] is True and d["check_rel_l2"] is not None
    assert d["roofline"]["kernels"] and d["roofline"]["dominant_kernel"]["name"] in d["roofline"]["kernels"]
    assert d["cpu_baseline"]["value"] > 0
