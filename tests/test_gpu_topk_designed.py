"""The batched radix top-k (k_btk_hist, k_btk_digit, k_btk_ties, k_btk_scan,
k_btk_select, k_btk_final) on the designed inputs of tests/topk_cases.py,
against the stable-argsort reference topk_cases.topk_ref, which the reference
implementation's own results confirm on every tie-free case
(tests/golden/topk_designed.json, test_topk_cases_cpu.py).

Each group is one ofl_sparsify_topk_batch call over an arena whose gaps and
output are pre-filled: sparse arrays bit-identical (uint32 views), n_pos, n_neg,
n_zero, shifted and kept_min exact, a second run bit-identical, every gap
element untouched.  abs_sum is within 1e-12 relative of the exact (fsum) value:
its terms share one sign and the device chains fewer than 300 dependent float64
adds (256 per thread, 8 tree levels, under 10 in k_btk_final), at most 3.3e-14
relative, so the bar keeps a 30x margin.

Slowest test on an MI355X: test_digit_cases_one_arena, 1.9 s (of which most is the
host's stable argsorts); test_long_cases 1.7 s; the module 7 s.
"""
import functools
import gzip
import json
import os

import numpy as np
import pytest
import torch

from tests import topk_cases as C
from tests.golden_io import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _ref(build, args):
    x, k, _ = build(*args)
    return C.topk_ref(x, k)


def _run_batch(cases, mods=None):
    """cases: [(builder, args)].  Runs the batch twice and checks everything the
    module docstring lists; -> per-tensor device stats."""
    from openfl_amd import lossy
    built = [build(*args) for build, args in cases]
    xs, ks = [b[0] for b in built], [b[1] for b in built]
    a, offs, gap = C.arena(xs, mods)
    x_dev = torch.from_numpy(a).to(DEV)
    sentinel = np.full(a.size, C.SENTINEL, np.uint32)
    res = []
    for _ in range(2):
        out = torch.from_numpy(sentinel.view(np.float32).copy()).to(DEV)
        st = lossy.sparsify_topk_batch(x_dev, offs, [x.size for x in xs], ks, out)
        res.append((out.cpu().numpy().view(np.uint32), st))
    out, st = res[0]
    np.testing.assert_array_equal(out, res[1][0])
    np.testing.assert_array_equal(out[gap], sentinel[gap])
    bad = []                                                     # every failing (case, what): a failure names its branches
    for t, ((build, args), x, o, k) in enumerate(zip(cases, xs, offs, ks)):
        sp, ref = _ref(build, args)
        tag = f"{build.__name__}{args}"
        wrong = int(np.sum(out[o:o + x.size] != sp.view(np.uint32)))
        if wrong:
            bad.append((tag, "sparse", wrong))
        for key in ("n_pos", "n_neg", "n_zero", "shifted", "kept_min"):
            if not st[key][t] == ref[key]:
                bad.append((tag, key, st[key][t], ref[key]))
        if np.isinf(ref["abs_sum"]):
            ok = st["abs_sum"][t] == ref["abs_sum"]
        else:
            ok = abs(st["abs_sum"][t] - ref["abs_sum"]) <= 1e-12 * max(ref["abs_sum"], 1e-30)
        if not ok:
            bad.append((tag, "abs_sum", st["abs_sum"][t], ref["abs_sum"]))
        for key in ("n_pos", "n_neg", "n_zero", "shifted", "kept_min", "abs_sum"):
            if not res[1][1][key][t] == st[key][t]:
                bad.append((tag, key, "second run differs"))
    assert not bad, (len(bad), bad[:40])
    return st, offs


def test_digit_cases_one_arena():
    """Every digit design as one tensor of one arena: each pass stops in the
    bottom, top and an interior bin of a lane, in lane 0 and lane 63, with the
    bin's cumulative count equal to and above `need`; thresholds from denormals
    to the last finite digit; ~190 tensors through tensor_of's search."""
    names = C.digit_names()
    _, offs = _run_batch([(C.digit, nm) for nm in names])
    assert {o % 4 for o in offs} == {0, 1, 2, 3}


def _tie_group(build, names):
    st, _ = _run_batch([(build, (nm,)) for nm in names])
    for t, nm in enumerate(names):
        facts = build(nm)[2]
        # the negative tie is kept iff its global rank < the ties kept: it alone decides sign and shift
        assert st["kept_min"][t] == facts["kept_min"], (nm, st["kept_min"][t])
        assert st["shifted"][t] == facts["shifted"], nm


def test_tie_cases():
    """Cuts inside each block and on block boundaries, all ties or all but one
    kept, the single negative tie at rank need - 1 and need, before, in and
    after the cut's block, and a wave-dense run of ties."""
    _tie_group(C.tie, C.tie_names())


def test_long_cases():
    """67 blocks per tensor: the second trip of k_btk_scan's and k_btk_final's
    block loops, the tie prefix carried into blocks 64 and 65."""
    _tie_group(C.long, C.long_names())


def test_shift_edges():
    names = C.edge_names()
    st, _ = _run_batch([(C.edge, (nm,)) for nm in names])
    for t, nm in enumerate(names):
        facts = C.edge(nm)[2]
        assert st["shifted"][t] == facts["shifted"] and st["n_zero"][t] == facts["n_zero"], nm


def test_zero_threshold():
    names = C.zero_names()
    st, _ = _run_batch([(C.zero, (nm,)) for nm in names])
    for t, nm in enumerate(names):
        assert st["n_pos"][t] == C.zero(nm)[2]["n_pos"] and st["shifted"][t], nm


def test_infinities():
    names = C.inf_names()
    st, _ = _run_batch([(C.inf, (nm,)) for nm in names])
    assert np.all(np.isinf(st["abs_sum"]))


def test_alignment_batch():
    """n in {1, 2, 3, 4, 5, 7, 65535, 65536, 65537} at arena offsets = 0, 1, 2, 3
    mod 4, k in {1, n}: btk_visit's head and tail at every alignment."""
    names = C.align_names()
    _, offs = _run_batch([(C.align, nm) for nm in names], [nm[1] for nm in names])
    assert [o % 4 for o in offs] == [nm[1] for nm in names]


def test_stc_chain_on_fixture_cases():
    """STCPipeline.forward on every fixture case (p = 1.0 cases included): the
    payload gunzips to the reference's ranks and the ternary table is the
    reference's, values to 1e-12 relative as in test_stc_vs_reference."""
    from openfl_amd.pipelines.stc_pipeline import STCPipeline
    with open(os.path.join(GOLDEN, "topk_designed.json")) as f:
        fx = {c["id"]: c for c in json.load(f)["cases"]}
    cases = C.fixture_cases()
    assert sorted(fx) == sorted(cid for cid, _, _ in cases)
    for cid, build, args in cases:
        x, k, _ = build(*args)
        rec = fx[cid]
        p = 1.0 if k == x.size else C.p_for(x.size, k)
        payload, mds = STCPipeline(p_sparsity=p, device=DEV).forward(np.array(x))
        ranks = np.frombuffer(gzip.decompress(payload), np.float32)
        assert C.sha(ranks.astype(np.int32)) == rec["ranks_sha256"], cid
        want = {int(r): v for r, v in rec["int_to_float"]}
        got = mds[1]["int_to_float"]
        assert sorted(got) == sorted(want), cid
        for r in want:
            np.testing.assert_allclose(got[r], want[r], rtol=1e-12, err_msg=cid)
