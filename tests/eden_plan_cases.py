"""Designed batches for the Eden planner's CPU check (tests/test_eden_plan_cpu.py):
each reaches a decision of openfl_amd/csrc/eden_plan.h -- a kernel, a table,
the wave cut, the split five-pass slice.  Data only; knobs not given are the
library's defaults (128 MiB waves, two streams, everything else automatic)."""

DEFAULTS = {"n_bits": 8, "wave_mib": 128, "streams": 2, "row2": -1, "pair": -1, "sset": -1, "fuse": -1, "dims": None}
WORKLOAD_CASES = ("resnet50_fp32", "mnist_cnn", "uniform_1gib", "llama3_8b_fp32_update")


def _case(name, numels, **knobs):
    assert not set(knobs) - set(DEFAULTS), knobs
    return dict(DEFAULTS, name=name, numels=list(numels), **knobs)


def cases():
    from openfl_amd.workloads import WORKLOADS, numel
    small = [5, 300, 1000, 2048, 5000, 10000, 20000, 32768]
    multi = [1 << 16, 1 << 18, 1 << 21, 5000, 300]
    waves = [1 << 22] * 6 + [1000, 1 << 20]
    out = [
        # tiny / small slices only: the small-set launch, or K_TINY and every K_SMALL size
        _case("small_sset", small), _case("small_sset0", small, sset=0),
        # k_col_multi and the launch fused with the small-set groups
        _case("multi_s2", multi, streams=2), _case("multi_fuse0", multi, fuse=0),
        _case("multi_sset0", multi, sset=0), _case("multi_bits1", multi, n_bits=1),
    ]
    # single heights: k_col to 6, k_col6 for 7..10, perm = 1 at 10
    out += [_case(f"height_{r}", [1 << (15 + r)]) for r in range(1, 11)]
    # two column levels, unsplit
    out += [_case(f"two_level_{p}", [1 << p], wave_mib=0) for p in (26, 27, 28, 29)]
    # the split five-pass slice: every row2 x pair mode, and the other heights (2^28: the nt middle pass)
    out += [_case(f"split_26_row2_{r}_pair_{q}".replace("-1", "a"), [1 << 26], wave_mib=64, streams=1, row2=r, pair=q)
            for r in (-1, 0, 1) for q in (-1, 0, 1)]
    out += [_case(f"split_{p}", [1 << p]) for p in (27, 28, 29)]
    # waves, one and two streams
    out += [_case(f"waves_{w}_s{s}", waves, wave_mib=w, streams=s) for w in (0, 32) for s in (1, 2)]
    out.append(_case("wave_of_its_own", [1 << 25, 1 << 22], wave_mib=16, streams=1))
    # the two-wave cut, and the benchmark's workloads
    sizes = {w: [numel(s) for _, s in WORKLOADS[w]()] for w in WORKLOAD_CASES}
    out.append(_case("resnet50_cut", sizes["resnet50_fp32"], streams=2, sset=0))
    out += [_case(w, sizes[w]) for w in WORKLOAD_CASES]
    # plane rows off the 8-byte grid: decode row A without 8-byte plane words
    out.append(_case("unaligned_planes", [65544], dims=[[8, 1 << 16]]))
    # more row tiles in one launch than a row table holds
    out.append(_case("above_row_tab_max", [1 << 29] * 5, wave_mib=0, streams=1))
    return out


def to_line(c):
    """One case as a line of tests/eden_plan_check.cpp's input."""
    f = [c["name"], c["n_bits"], c["wave_mib"], c["streams"], c["row2"], c["pair"], c["sset"], c["fuse"],
         len(c["numels"]), *c["numels"]]
    if c["dims"] is None:
        f.append(0)
    else:
        f += [1, *[len(d) for d in c["dims"]], *[v for d in c["dims"] for v in d]]
    return " ".join(str(v) for v in f)
