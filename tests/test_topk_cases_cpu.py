"""The designs of tests/topk_cases.py hold what they claim, checked on the host.

A numpy restatement of the three-pass radix select (masks and counts per pass,
nothing of the kernels' lane structure beyond the bin numbering) recovers the
threshold, each pass's digit and `need` for every case; over all cases every
pass meets every branch class; the facts of the tie designs hold in the
stable-argsort reference; and that reference equals the fixture recorded from
the reference implementation (tests/golden/topk_designed.json)."""
import json
import os

import numpy as np
import pytest

from tests import topk_cases as C
from tests.golden_io import GOLDEN


def radix_select(x, k):
    """-> (T pattern, ties at T to keep, per pass: digit, need before, bin class)."""
    m = x.view(np.uint32) & np.uint32(0x7FFFFFFF)
    cand = np.ones(x.size, bool)
    need, prefix, trace = k, 0, []
    for p in range(3):
        nb = 1 << C.WIDTH[p]
        dig = (m >> np.uint32(C.SHIFT[p])) & np.uint32(nb - 1)
        h = np.bincount(dig[cand], minlength=nb).astype(np.int64)
        above = np.cumsum(h[::-1])[::-1] - h                    # candidates in higher bins
        d = int(np.nonzero(above + h >= need)[0].max())
        trace.append({"digit": d, "need": need, "lane": d // C.PER[p], "pos": C._position(d, C.PER[p]),
                      "cmp": "==" if above[d] + h[d] == need else ">"})
        cand &= dig == d
        need -= int(above[d])
        prefix |= d << C.SHIFT[p]
    return prefix, need, trace


def kth_pattern(x, k):
    m = np.sort(x.view(np.uint32) & np.uint32(0x7FFFFFFF))
    return int(m[x.size - k]), int(np.sum(m == m[x.size - k]))


def classes(trace, p):
    t = trace[p]
    out = {t["pos"], t["cmp"]}
    if t["lane"] in (0, 63):
        out.add(f"lane{t['lane']}")
    return out


ALL_CLASSES = {"bottom", "top", "interior", "lane0", "lane63", "==", ">"}


def test_digit_cases_recovered_and_every_branch_class_met():
    seen = [set(), set(), set()]
    for nm in C.digit_names():
        x, k, facts = C.digit(*nm)
        assert x.size == C.DIGIT_N and x.dtype == np.float32
        T, ties = kth_pattern(x, k)
        assert T == facts["T"] and ties == 1, nm                 # tie-free: the threshold magnitude is unique
        assert k == int(np.sum((x.view(np.uint32) & 0x7FFFFFFF) > T)) + 1
        got_T, need, trace = radix_select(x, k)
        assert got_T == T and need == 1, nm
        for p in range(3):
            want = facts["passes"][p]
            assert {key: trace[p][key] for key in want} == want, (nm, p)
            seen[p] |= classes(trace, p)
        if nm[3] is not None:                                    # T the smallest of its bin in that pass
            assert trace[nm[3]]["cmp"] == "==", nm
    # distinct magnitudes put one element into a pass-2 bin, so its count meets
    # `need` exactly there; a count above `need` in pass 2 takes ties
    for build, names in ((C.tie, C.tie_names()), (C.zero, C.zero_names())):
        for nm in names:
            x, k, facts = build(nm)
            got_T, need, trace = radix_select(x, k)
            assert got_T == facts["T"] and need == facts["need"], nm
            for p in range(3):
                seen[p] |= classes(trace, p)
    for p in range(3):
        assert seen[p] == ALL_CLASSES, (p, ALL_CLASSES - seen[p])


def test_digit_table_size():
    names = C.digit_names()
    assert len(set(names)) == len(names) and 180 <= len(names) <= 200


@pytest.mark.parametrize("name", C.tie_names())
def test_tie_case_facts(name):
    x, k, facts = C.tie(name)
    _check_tie_facts(x, k, facts, C.TIE_N)


@pytest.mark.parametrize("name", C.long_names())
def test_long_case_facts(name):
    x, k, facts = C.long(name)
    assert x.size == 66 * C.BLOCK + 3 and 9_000 <= k <= 11_000
    assert sorted(set(facts["tie_idx"] // C.BLOCK)) == [0, 63, 64, 65]
    assert facts["cut_block"] in (64, 65) and facts["neg_block"] == 64
    _check_tie_facts(x, k, facts, C.LONG_N)


def _check_tie_facts(x, k, facts, n):
    assert x.size == n
    T, ties = kth_pattern(x, k)
    assert T == C.HALF and ties == facts["ties"]
    tie_idx = np.nonzero(np.abs(x) == np.float32(0.5))[0]
    np.testing.assert_array_equal(tie_idx, facts["tie_idx"])
    sure = np.abs(x) > np.float32(0.5)
    assert np.all(x[sure] >= 1.0) and k == int(sure.sum()) + facts["need"]
    small = np.abs(x[np.abs(x) < np.float32(0.5)])
    assert np.unique(small).size == small.size
    sp, ref = C.topk_ref(x, k)
    kept_ties = np.nonzero(sp[tie_idx])[0]
    np.testing.assert_array_equal(kept_ties, np.arange(facts["need"]))   # lowest index first
    # the block of the cut: the one whose ties are partly kept
    per_block = np.bincount(tie_idx // C.BLOCK, minlength=(n + C.BLOCK - 1) // C.BLOCK)
    kept_block = np.bincount(tie_idx[:facts["need"]] // C.BLOCK, minlength=per_block.size)
    partial = [int(b) for b in np.nonzero((kept_block > 0) & (kept_block < per_block))[0]]
    assert partial == ([] if facts["cut_block"] is None else [facts["cut_block"]])
    neg = np.nonzero(x[tie_idx] < 0)[0]
    assert list(neg) == ([] if facts["neg_rank"] is None else [facts["neg_rank"]])
    if neg.size:
        assert tie_idx[neg[0]] // C.BLOCK == facts["neg_block"]
    neg_kept = bool(neg.size and neg[0] < facts["need"])
    assert ref["shifted"] == facts["shifted"] == neg_kept         # the one negative tie decides the shift
    assert ref["kept_min"] == facts["kept_min"] == np.float32(-0.5 if neg_kept else 0.5)


def test_tie_table_covers_the_listed_variants():
    f = {nm: C.tie(nm)[2] for nm in C.tie_names()}
    assert {f[nm]["cut_block"] for nm in ("cut_b0", "cut_b1", "cut_b2")} == {0, 1, 2}
    assert f["cut_boundary_01"]["cut_block"] is None and f["cut_boundary_01"]["need"] == 300
    assert f["all_kept"]["need"] == f["all_kept"]["ties"] and f["short_one"]["need"] == f["short_one"]["ties"] - 1
    one = f["neg_kept_last_in_cut"]
    assert one["neg_rank"] == one["need"] - 1 and one["neg_block"] == one["cut_block"] and one["shifted"]
    one = f["neg_dropped_first_in_cut"]
    assert one["neg_rank"] == one["need"] and one["neg_block"] == one["cut_block"] and not one["shifted"]
    assert f["neg_earlier_block"]["neg_block"] < f["neg_earlier_block"]["cut_block"]
    assert f["neg_later_block"]["neg_block"] > f["neg_later_block"]["cut_block"]
    one = f["neg_dropped_first_on_boundary"]
    assert one["neg_rank"] == one["need"] and one["cut_block"] is None and not one["shifted"]
    x = C.tie(C.DENSE)[0]
    run = f[C.DENSE]["tie_idx"][:64]
    assert np.all(np.diff(run) == 1) and run[0] % 64 == 0 and np.all(x[run] == np.float32(0.5))
    long = {nm: C.long(nm)[2] for nm in C.long_names()}
    assert {v["cut_block"] for v in long.values()} == {64, 65}
    assert {v["shifted"] for v in long.values() if v["cut_block"] == 64} == {True, False}


@pytest.mark.parametrize("name", C.edge_names())
def test_shift_edge_cases(name):
    x, k, facts = C.edge(name)
    assert kth_pattern(x, k)[1] == 1
    sp, ref = C.topk_ref(x, k)
    assert ref["kept_min"] == facts["kept_min"] and ref["shifted"] == facts["shifted"]
    assert ref["n_zero"] == facts["n_zero"] and ref["n_pos"] + ref["n_neg"] + ref["n_zero"] == k
    if name == "min_1em7":
        assert ref["kept_min"] == np.float32(1e-7) and not ref["shifted"]
    if name == "min_below_1em7":
        assert ref["kept_min"] == np.nextafter(np.float32(1e-7), np.float32(0)) and ref["shifted"]
    if name == "min_minus_1em7":
        at = np.nonzero(x == -np.float32(1e-7))[0]
        assert ref["kept_min"] == -np.float32(1e-7) and at.size == 1 and ref["n_neg"] == 0
        assert sp[at[0]].view(np.uint32) == 0 and np.count_nonzero(sp) == k - 1     # kept, and exactly +0.0
    if name == "all_negative":
        assert ref["n_neg"] == k and ref["shifted"]
    if name == C.EDGE_DENORMAL:
        assert ref["kept_min"].view(np.uint32) == 1 and ref["n_pos"] == k


@pytest.mark.parametrize("name", C.zero_names())
def test_zero_threshold_cases(name):
    x, k, facts = C.zero(name)
    assert kth_pattern(x, k) == (0, C.ZERO_N - 100) and k > np.count_nonzero(x)
    zeros = x[x == 0].view(np.uint32)
    assert 0 < np.count_nonzero(zeros) < zeros.size              # both +0.0 and -0.0
    sp, ref = C.topk_ref(x, k)
    np.testing.assert_array_equal(np.nonzero(sp == np.float32(1e-7))[0], facts["kept_zeros"])
    assert ref["shifted"] and ref["n_pos"] == facts["n_pos"] == k and ref["n_neg"] == ref["n_zero"] == 0
    first = facts["kept_zeros"][0] // C.BLOCK, facts["kept_zeros"][-1] // C.BLOCK
    assert first == {"cut_b0": (0, 0), "cut_b1": (0, 1), "all": (0, 1)}[name]


@pytest.mark.parametrize("name", C.inf_names())
def test_infinity_cases(name):
    x, k, facts = C.inf(name)
    assert np.sum(np.isinf(x)) == facts["n_inf"] < k and not np.any(np.isnan(x))
    assert kth_pattern(x, k)[1] == 1
    sp, ref = C.topk_ref(x, k)
    assert ref["abs_sum"] == np.inf and ref["shifted"] == facts["shifted"]
    assert np.sum(np.isinf(sp)) == facts["n_inf"]


@pytest.mark.parametrize("name", C.full_names())
def test_full_cases(name):
    x, k, facts = C.full(name)
    assert k == x.size == int(np.ceil(x.size * 1.0))
    sp, ref = C.topk_ref(x, k)
    ranks, table = C.ternary_ref(sp)
    assert tuple(np.sign(v) for v in table.values()) == facts["classes"] and ref["shifted"] == facts["shifted"]
    assert sorted(np.unique(ranks)) == list(range(len(facts["classes"])))


def test_alignment_cases():
    names = C.align_names()
    assert {n for n, _, _ in names} == {1, 2, 3, 4, 5, 7, 65535, 65536, 65537}
    xs = [C.align(*nm)[0] for nm in names]
    a, offs, gap = C.arena(xs, [nm[1] for nm in names])
    for nm, x, o in zip(names, xs, offs):
        assert o % 4 == nm[1] and x.size == nm[0] and nm[2] in (1, nm[0])
        assert np.unique(np.abs(x)).size == x.size
        np.testing.assert_array_equal(a[o:o + x.size], x)
        assert gap[o - 1] and gap[o + x.size] and not gap[o:o + x.size].any()
    assert gap.sum() == a.size - sum(x.size for x in xs)


def test_plain_arena_offsets_hit_every_alignment():
    xs = [np.zeros(C.DIGIT_N, np.float32)] * 12
    _, offs, gap = C.arena(xs)
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    assert all(gap[o - 1] and gap[o + C.DIGIT_N] for o in offs)


def test_p_for():
    for n, k in ((C.DIGIT_N, 1), (C.DIGIT_N, C.DIGIT_N), (C.DIGIT_N, 33_333), (777, 100), (5000, 50), (3000, 3000)):
        assert int(np.ceil(n * C.p_for(n, k))) == k


def test_reference_equals_recorded_fixture():
    with open(os.path.join(GOLDEN, "topk_designed.json")) as f:
        fx = {c["id"]: c for c in json.load(f)["cases"]}
    cases = C.fixture_cases()
    assert sorted(fx) == sorted(cid for cid, _, _ in cases)
    for cid, build, args in cases:
        x, k, _ = build(*args)
        rec = fx[cid]
        sp, ref = C.topk_ref(x, k)
        assert (rec["n"], rec["k"]) == (x.size, k), cid
        assert rec["sparse_sha256"] == C.sha(sp), cid
        assert rec["kept"] == k and rec["shifted"] == ref["shifted"], cid
        ranks, table = C.ternary_ref(sp)
        assert rec["ranks_sha256"] == C.sha(ranks), cid
        want = {int(r): v for r, v in rec["int_to_float"]}
        assert sorted(want) == sorted(table), cid
        for r in want:
            np.testing.assert_allclose(table[r], want[r], rtol=1e-12, err_msg=cid)
