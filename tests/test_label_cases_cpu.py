"""The designs of tests/label_cases.py hold what they claim, checked on the host:
the two formulations of the reference agree on every case, every rule's probes
reach every cluster and sit on every finite midpoint, the layouts have the
record, chunk and segment counts the device tests rely on, and the chain
tensors chain as far as they say."""
import hashlib
import importlib

import numpy as np
import pytest

from tests import label_cases as C


def test_rules_keep_the_contract():
    assert len(C.RULES) == 13
    for name, m in C.RULES.items():
        assert m.dtype == np.float32 and m.shape == (8,) and m[7] == np.inf, name
        assert np.all(m[1:] >= m[:-1]), name
    assert [int(np.sum(np.isfinite(C.RULES[f"k{k}"]))) for k in range(1, 9)] == list(range(8))
    assert np.sum(C.RULES["dup2"] == 0.5) == 2 and np.sum(C.RULES["dup3"] == 0.5) == 3
    assert C.RULES["ternary"][:3].view(np.uint32).tolist() == [0x80000001, 0, 0x7F800000]
    assert {-C.FLT_MAX, C.FLT_MAX} <= set(C.RULES["fltmax"].tolist())
    den = C.RULES["denormal"][:3]
    assert np.all(den != 0) and np.all(np.abs(den) < np.finfo(np.float32).tiny)
    vals = np.concatenate(C.VALUE_SETS)
    for want in (0x80000000, 0, 0x7F800000, 0xFF800000):                       # -0.0, +0.0, +inf, -inf
        assert want in vals.view(np.uint32)
    assert np.any((vals != 0) & (np.abs(vals) < np.finfo(np.float32).tiny))   # a denormal
    assert np.any(vals != np.round(vals))
    assert all(np.any(v[1:] == v[:-1]) for v in C.VALUE_SETS[1:])             # adjacent clusters, one value
    for r in C.RANK_SETS:
        assert np.all(r == np.round(r)) and r.min() >= 0 and r.max() == 31
        assert np.unique(r).size < 8 and np.any(np.diff(r) < 0) and np.any(np.diff(r) > 0)


@pytest.mark.parametrize("rule", C.RULE_NAMES)
def test_probes_reach_every_cluster_and_every_midpoint(rule):
    m, p, pat = C.RULES[rule], C.probes(rule), C.pattern(rule)
    assert pat.size == C.PATTERN and p.size < C.PATTERN
    idx = C.label_index(p, m)
    np.testing.assert_array_equal(idx, C.label_index_sorted(p, m))
    assert set(idx.tolist()) == C.reachable(m), rule
    for j, v in enumerate(m[np.isfinite(m)]):
        on = p == v
        assert on.any(), (rule, v)
        # on the midpoint: the lower cluster; one float32 above it: the cluster above every equal midpoint
        assert np.all(idx[on] == np.sum(m[:7] < v))
        with np.errstate(over="ignore"):
            up = np.nextafter(v, np.float32(np.inf))
        assert np.all(idx[p.view(np.uint32) == up.view(np.uint32)] == np.sum(m[:7] <= v)), (rule, v)
    assert np.all(idx[np.isnan(p)] == 0) and np.sum(np.isnan(p)) == 2
    assert np.signbit(p[np.isnan(p)]).tolist() == [False, True]
    for bits in (0, 0x80000000, 1, 0x80000001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000):
        assert bits in p.view(np.uint32), (rule, hex(bits))
    assert set(p.view(np.uint32).tolist()) <= set(pat.view(np.uint32).tolist())   # the pattern: probes and filler


def test_ternary_rule_is_the_sign():
    p = C.probes("ternary")
    idx = C.label_index(p, C.RULES["ternary"])
    ok = ~np.isnan(p)
    np.testing.assert_array_equal(idx[ok], np.sign(p[ok]).astype(np.int64) + 1)


@pytest.mark.parametrize("name", C.APPLY_LAYOUTS)
def test_apply_cases(name):
    starts, ends, n = C.apply_layout(name)
    assert n < 1_000_000
    assert np.all(starts >= 0) and np.all(ends <= n) and np.all(ends >= starts) and np.all(starts[1:] >= ends[:-1])
    for rot in range(len(C.VALUE_SETS)):
        x, recs, base = C.apply_case(name, rot)
        assert x.size == base.size == n and np.all(np.isfinite(base) | np.isinf(base))
        for with_base in (base, None):
            a, inside = C.applied(x, recs, with_base)
            b, inside_b = C.applied(x, recs, with_base, C.label_index_sorted)
            assert C.same_bits(a, b) == 0 and np.array_equal(inside, inside_b)
            assert np.all(a.view(np.uint32)[~inside] == C.SENTINEL)
            assert not np.any(a.view(np.uint32)[inside] == C.SENTINEL)
        assert inside.sum() == int((ends - starts).sum())
        for t, r in enumerate(recs):
            if r["end"] - r["start"] >= 64:
                assert np.isnan(x[r["start"]:r["end"]]).any(), (name, t)
        if len(recs) > 1:   # neighbouring records differ in rule, and over the rotations every value set is used
            assert not any(np.array_equal(recs["mid"][t], recs["mid"][t + 1]) for t in range(len(recs) - 1))
    used = {recs_["rank"][0].tobytes() for recs_ in (C.apply_case(name, rot)[1] for rot in range(3))}
    assert len(used) == 3


def test_apply_layout_facts():
    s, e, _ = C.apply_layout("short")
    assert sorted(zip((s % 4).tolist(), (e - s).tolist())) == sorted((m, n) for m in range(4) for n in C.SHORT_LENGTHS)
    s, e, _ = C.apply_layout("chunks")
    assert (s % 4).tolist() == [0] * 4 + [1] * 4
    assert C.chunk_counts(C.apply_case("chunks")[1]).tolist() == [1, 1, 2, 3] * 2
    for n in C.COUNTS:
        s, e, _ = C.apply_layout(f"counts/{n}")
        assert s.size == n and set((e - s).tolist()) <= {1, 2, 3, 4, 5}
        if n > 1:
            assert set((s[1:] - e[:-1]).tolist()) <= {0, 1, 2, 3}
        if n >= 63:
            assert set((e - s).tolist()) == {1, 2, 3, 4, 5} and set((s[1:] - e[:-1]).tolist()) == {0, 1, 2, 3}
    assert C.chunk_counts(C.apply_case("counts/4160")[1]).sum() >= 4096
    assert [n > C.MAX_T for n in C.COUNTS] == [False] * 7 + [True] * 2 and C.MAX_T in C.COUNTS
    empty = {k: np.flatnonzero(np.subtract(*C.apply_layout(f"empty/{k}")[1::-1]) == 0).tolist() for k in C.EMPTY_KINDS}
    nt = C.apply_layout("empty/first")[0].size
    assert empty["first"] == [0] and empty["last"] == [nt - 1] and empty["middle"] == [nt // 2]
    assert empty["run70"] == list(range(100, 170)) and 70 > (nt + 63) // 64      # longer than a lane's share of the scan
    assert empty["around4096"] == [C.MAX_T - 1, C.MAX_T] and C.apply_layout("empty/around4096")[0].size > C.MAX_T + 64
    s, e, _ = C.apply_layout("empty/only")
    assert s.size == 5 and np.all(s == e)
    assert not C.applied(*C.apply_case("empty/only")[:2], None)[1].any()          # nothing is written


@pytest.mark.parametrize("name", C.ENCODER_LAYOUTS)
def test_encoder_cases(name):
    for one_off in (False, True):
        x, recs = C.encoder_case(name, one_off)
        s, e = recs["start"], recs["end"]
        assert s[0] >= 1 - one_off and e[-1] < x.size                           # a leading and a trailing gap
        assert np.all(e > s) and np.all(s[1:] >= e[:-1])
        ranks = C.ranks_of(x, recs)
        np.testing.assert_array_equal(ranks, C.ranks_of(x, recs, C.label_index_sorted))
        assert np.all(ranks == np.round(ranks)) and ranks.min() >= 0 and ranks.max() <= 31
        inside = np.zeros(x.size, bool)
        for a, b in zip(s, e):
            inside[a:b] = True
        gap = x[~inside]
        assert np.all(ranks[~inside] == 0)
        assert np.all(np.isnan(gap) | np.isin(gap, [np.inf, 32.0, 2.5]))        # nothing in a gap is a rank
        if gap.size >= 8:
            assert np.isnan(gap).any() and (gap == 32.0).any() and (gap == 2.5).any() and np.isinf(gap).any()
        assert np.count_nonzero(ranks[inside]) > 0.9 * inside.sum()              # a record taken for a gap shows
    full = C.encoder_case(name)[0]
    assert np.array_equal(full[1:].view(np.uint32), x.view(np.uint32))


def test_encoder_layout_facts():
    for b in C.EDGES:
        s, e, _ = C.encoder_layout(f"edges/{b}/adjacent")
        assert e[0] == b == s[1]
        assert C.encoder_layout(f"edges/{b}/end")[1][0] == b and C.encoder_layout(f"edges/{b}/end")[0][1] > b
        assert C.encoder_layout(f"edges/{b}/begin")[0][1] == b and C.encoder_layout(f"edges/{b}/begin")[1][0] < b
    s, e, _ = C.encoder_layout("edges/span3")
    assert s[1] // C.MEMBER == 0 and (e[1] - 1) // C.MEMBER == 2
    for n in C.WINDOWS:
        s, e, _ = C.encoder_layout(f"window/{n}")
        seg = C.window_segment(n)
        assert s.size == n + 1 and np.all(s[:n] // C.SEG == seg) and np.all((e[:n] - 1) // C.SEG == seg)
        assert set((e[:n] - s[:n]).tolist()) <= set(range(1, 7))
        assert s[n] // C.SEG == seg + 1 and e[n] - s[n] > C.SEG               # the long record of the next segment
    s, e, _ = C.encoder_layout("octet")
    for at in C.OCTET_AT:
        assert (4 * at) % 32 == 0
        inside = (s >= at) & (e <= at + C.PER)
        assert inside.sum() >= 5 and set((e - s)[inside].tolist()) == {1, 2}
        assert s[inside].min() == at and e[inside].max() == at + C.PER
    assert C.encoder_layout("single")[0].size == 1


@pytest.mark.parametrize("bad", (32.0, 2.5))
def test_refused_case_reaches_the_bad_rank(bad):
    x, recs = C.refused_case(bad)
    assert bad in C.ranks_of(x, recs)
    assert bad not in C.ranks_of(*C.encoder_case("single"))


def test_chains():
    ranks = np.arange(8, dtype=np.float32)
    for name in C.CHAIN_NAMES:
        uniq, x = np.array(C.CHAINS[name], np.float32), C.chain_tensor(name)
        assert np.all(np.diff(uniq) > 0) and uniq.size <= C.CHAIN_K
        assert np.array_equal(np.unique(x), uniq) and x.size == uniq.size * C.CHAIN_REPEAT
    dec = {name: C.chain_ref(ranks, np.array(C.CHAINS[name], np.float32)) for name in C.CHAIN_NAMES}
    assert dec["full"].tolist() == [9.0] * 6 + [6.0, 7.0]
    assert dec["partial"].tolist() == [2.5, 2.5, 2.5, 7.0, 8.0, 9.5, 6.0, 7.0]
    assert dec["earlier"].tolist() == [-0.5, 0.0, 1.0, 2.0, 3.0, 3.5, 6.0, 7.0]
    assert dec["none"].tolist() == list(C.CHAINS["none"]) + [6.0, 7.0]
    assert dec["fewer"].tolist() == [7.5, 7.5, 7.5, 3.0, 4.0, 5.0, 6.0, 7.0]
    stable = C.chain_until_stable(ranks, np.array(C.CHAINS["earlier"], np.float32))
    assert stable.tolist() == [-0.5] * 5 + [3.5, 6.0, 7.0] and not np.array_equal(stable, dec["earlier"])
    # a map no fit returns (uniq ascends), for the loop alone: 0 equals an earlier key and stays, 3 a later one
    assert C.chain_ref(ranks[:4], np.float32([0.5, 0.0, 3.0, 2.0])).tolist() == [0.5, 0.0, 2.0, 2.0]
    assert C.chain_until_stable(ranks[:4], np.float32([0.5, 0.0, 3.0, 2.0])).tolist() == [0.5, 0.5, 2.0, 2.0]


def _digest(mod):
    h = hashlib.sha256()
    for name in mod.APPLY_LAYOUTS:
        for a in mod.apply_case(name, 1):
            h.update(np.ascontiguousarray(a).tobytes())
    for name in mod.ENCODER_LAYOUTS:
        for a in mod.encoder_case(name, True):
            h.update(np.ascontiguousarray(a).tobytes())
    for name in mod.CHAIN_NAMES:
        h.update(mod.chain_tensor(name).tobytes())
    return h.hexdigest()


def test_module_is_deterministic():
    first = _digest(C)
    again = importlib.reload(importlib.import_module("tests.label_cases"))
    assert _digest(again) == first
