"""Designed inputs of the batched radix top-k (k_btk_* in csrc/lossy_topk.h)
and the numpy reference they are compared with.  numpy only, no tests: the
designs are checked on the host by test_topk_cases_cpu.py and run on the device
by test_gpu_topk_designed.py.

Every builder is deterministic, builds its values from uint32 bit patterns and
returns (x float32 read-only, k, facts).  The threshold T is the bit pattern of
the k-th largest |x|; its 11/11/9-bit digits (D0, D1, D2) are what the three
select passes find, 64 lanes of `per` = 32, 32, 8 bins each.
"""
import functools
import hashlib
import math

import numpy as np

BLOCK = 1 << 16                  # elements per device block (kBkmChunk)
SHIFT = (20, 9, 0)               # btk_shift
WIDTH = (11, 11, 9)              # btk_width
PER = (32, 32, 8)                # bins per lane in each pass
MAXP = 0x7F7FFFFF                # largest finite magnitude pattern
F1EM7 = np.float32(1e-7)         # the reference's 10e-8, as the float32 it is added as


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- reference ----------------------------------------------------------------
def topk_ref(x, k):
    """numpy restatement of SparsityTransformer._topk_func (skc_pipeline.py:
    72-94) with ties at the k-th magnitude kept lowest index first."""
    order = np.argsort(-np.abs(x), kind="stable")[:k]
    kept = np.zeros(x.size, bool)
    kept[order] = True
    shift = np.float32(1e-7) if np.min(x[kept]) < 1e-7 else np.float32(0)
    sp = np.where(kept, x + shift, np.float32(0)).astype(np.float32)
    v = sp[kept]
    return sp, {"n_pos": int(np.sum(v > 0)), "n_neg": int(np.sum(v < 0)), "n_zero": int(np.sum(v == 0)),
                "abs_sum": math.fsum(np.abs(v.astype(np.float64))), "shifted": bool(shift),
                "kept_min": np.min(x[kept])}


def ternary_ref(sp):
    """TernaryTransformer.forward (stc_pipeline.py:105-130) of a sparse array:
    -> (int32 ranks, {rank: value}) with the mean |x| from an exact sum."""
    m = math.fsum(np.abs(sp.astype(np.float64))) / sp.size
    sign = np.sign(sp).astype(np.int64)                       # -1, 0, +1
    present = [s for s in (-1, 0, 1) if np.any(sign == s)]
    rank_of = np.zeros(3, np.int32)
    for r, s in enumerate(present):
        rank_of[s + 1] = r
    return rank_of[sign + 1], {r: s * m if s else 0.0 for r, s in enumerate(present)}


def p_for(n, k):
    """A sparsity ratio p with ceil(n * p) == k, the count the pipelines keep."""
    for p in (k / n, (k - 0.5) / n):
        if int(np.ceil(n * p)) == k:
            return p
    raise AssertionError((n, k))


def _freeze(x):
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    return x


def _from_patterns(pats, rng):
    """float32 with the given magnitude patterns, random signs, shuffled."""
    pats = rng.permutation(np.asarray(pats, np.uint32))
    sign = rng.integers(0, 2, pats.size, dtype=np.uint32) << np.uint32(31)
    return (pats | sign).view(np.float32)


def _position(d, per):
    return "bottom" if d % per == 0 else ("top" if d % per == per - 1 else "interior")


# ---- digit cases --------------------------------------------------------------
DIGIT_N = BLOCK + 77             # two blocks add into one global histogram
D0S = (0, 1, 31, 32, 1023, 1024, 2015, 2016, 2039)   # 0: denormals, 2039 = 0x7F7: the last finite digit
D1S = (0, 1, 31, 32, 2047)
D2S = (0, 7, 8, 511)
# none of D2S is an interior bin of its pass-2 lane (per = 8): these add one
D2_INTERIOR = ((1, 1, 260), (1023, 31, 3), (2016, 32, 508))
# T the smallest pattern of its pass-0 / pass-1 bin: once where that bin is the
# bottom bin of its lane in both passes, once where it is not
LOW_VARIANTS = ((32, 32, 7), (1023, 1, 8))


def digit_names():
    names = []
    for d0 in D0S:
        for d1 in D1S:
            for d2 in D2S:
                t = d0 << 20 | d1 << 9 | d2
                if t != 0 and t != MAXP:
                    names.append((d0, d1, d2, None))
    names += [(d0, d1, d2, None) for d0, d1, d2 in D2_INTERIOR]
    names += [(d0, d1, d2, low) for d0, d1, d2 in LOW_VARIANTS for low in (0, 1)]
    return names


def digit_id(name):
    d0, d1, d2, low = name
    return f"d{d0}_{d1}_{d2}" + ("" if low is None else f"_low{low}")


@functools.lru_cache(maxsize=None)
def digit(d0, d1, d2, low=None):
    """Distinct magnitudes around T = d0<<20 | d1<<9 | d2, k = (count > T) + 1.
    low = 0 / 1 removes every smaller pattern of T's pass-0 / pass-1 bin, so that
    the bin's cumulative count meets `need` exactly."""
    T = d0 << 20 | d1 << 9 | d2
    assert 0 < T < MAXP
    rng = np.random.default_rng([d0, d1, d2, 0 if low is None else low + 1])
    near = {T}
    for j in range(1, 41):
        near |= {T - j, T + j}
    for j in range(1, 200):
        near |= {T - (j << 9), T + (j << 9), T - (j << 20), T + (j << 20)}
    near = np.array(sorted(p for p in near if 0 <= p <= MAXP), np.int64)
    fill = np.setdiff1d(np.unique(rng.integers(0, MAXP + 1, DIGIT_N + 4096)), near)

    def thin(p):
        if low is None:
            return p
        sh = SHIFT[low]
        return p[~((p >> sh == T >> sh) & (p < T))]

    near, fill = thin(near), rng.permutation(thin(fill))
    pats = np.concatenate([near, fill[:DIGIT_N - near.size]])
    assert pats.size == DIGIT_N and np.unique(pats).size == DIGIT_N
    x = _from_patterns(pats, rng)
    facts = {"T": T, "passes": []}
    for p in range(3):
        d = (T >> SHIFT[p]) & ((1 << WIDTH[p]) - 1)
        below = np.sum((pats >> SHIFT[p] == T >> SHIFT[p]) & (pats < T))
        facts["passes"].append({"digit": d, "lane": d // PER[p], "pos": _position(d, PER[p]),
                                "cmp": ">" if below else "=="})
    return _freeze(x), int(np.sum(pats > T)) + 1, facts


# ---- tie cases ----------------------------------------------------------------
HALF = 0x3F000000                # T = 0.5: digits (1008, 0, 0)
TIE_N = 2 * BLOCK + 1000         # three blocks


def _tie_case(n, ties_per_block, need, neg_rank, n_sure, seed):
    """ties_per_block: {block: in-block indices of the ties, ascending}.  The
    first `need` ties in index order are kept; tie number neg_rank (or none) is
    -0.5.  n_sure values >= 1, all positive, are kept for sure; every other
    element is a distinct magnitude below 0.5 with a random sign."""
    rng = np.random.default_rng(seed)
    small = rng.permutation(np.arange(1, n + 1)).astype(np.float32) * np.float32(2.0 ** -24)
    assert n < 1 << 23                                         # i * 2^-24 exact and < 0.5
    x = small * rng.choice(np.array([-1, 1], np.float32), n)
    tie_idx = np.concatenate([b * BLOCK + np.asarray(ix, np.int64) for b, ix in sorted(ties_per_block.items())])
    assert np.all(np.diff(tie_idx) > 0) and tie_idx[-1] < n and 0 < need <= tie_idx.size
    free = np.setdiff1d(np.arange(n), tie_idx)
    sure = rng.choice(free, n_sure, replace=False)
    x[sure] = np.float32(1.0) + np.arange(n_sure, dtype=np.float32) * np.float32(2.0 ** -12)
    x[tie_idx] = np.float32(0.5)
    if neg_rank is not None:
        x[tie_idx[neg_rank]] = np.float32(-0.5)
    counts = [len(ties_per_block.get(b, ())) for b in range((n + BLOCK - 1) // BLOCK)]
    base = np.concatenate([[0], np.cumsum(counts)])
    cut = [b for b in range(len(counts)) if base[b] < need < base[b + 1]]
    neg_kept = neg_rank is not None and neg_rank < need
    facts = {"T": HALF, "need": need, "ties": int(tie_idx.size), "tie_idx": tie_idx,
             "cut_block": cut[0] if cut else None,               # None: the cut lies on a block boundary
             "neg_rank": neg_rank, "neg_block": None if neg_rank is None else int(tie_idx[neg_rank] // BLOCK),
             "kept_min": np.float32(-0.5 if neg_kept else 0.5), "shifted": bool(neg_kept)}
    return _freeze(x), n_sure + need, facts


def _spread(count, lo, hi, step):
    ix = np.arange(lo, hi, step)[:count]
    assert ix.size == count
    return ix


def _three(c0, c1, c2):
    # block 2 holds 1000 elements
    return {0: _spread(c0, 11, BLOCK, 97), 1: _spread(c1, 5, BLOCK, 101), 2: _spread(c2, 1, 1000, 3)}


# name -> (ties in blocks 0, 1, 2; ties kept; rank of the one negative tie)
TIE_TABLE = {
    "cut_b0": ((300, 300, 100), 150, None),
    "cut_b1": ((300, 300, 100), 450, None),
    "cut_b2": ((300, 300, 100), 650, None),
    "cut_boundary_01": ((300, 300, 100), 300, None),           # need == block 0's ties: no boundary block
    "cut_boundary_12": ((250, 150, 100), 400, None),
    "all_kept": ((300, 300, 100), 700, None),
    "all_kept_neg_last": ((300, 300, 100), 700, 699),          # the kept minimum comes from the tie minimum
    "short_one": ((300, 300, 100), 699, None),
    "short_one_neg_last": ((200, 100, 300), 599, 599),         # the one dropped tie is the negative one
    "neg_kept_last_in_cut": ((200, 200, 200), 250, 249),       # rank need - 1, in the cut's block
    "neg_dropped_first_in_cut": ((100, 300, 50), 250, 250),    # rank need, in the cut's block
    "neg_earlier_block": ((50, 400, 10), 200, 20),
    "neg_later_block": ((120, 80, 300), 150, 250),
    "neg_kept_last_on_boundary": ((100, 100, 100), 100, 99),   # last tie of block 0, cut on the boundary
    "neg_dropped_first_on_boundary": ((100, 120, 90), 100, 100),   # first tie of block 1: base == need
    "neg_kept_first_of_block": ((150, 60, 70), 151, 150),      # first tie of the cut's block, the only one kept there
}
DENSE = "dense_wave"             # 64 consecutive ties: one wave's ballot sees >= 8 equal digits in passes 1 and 2


def tie_names():
    return list(TIE_TABLE) + [DENSE]


@functools.lru_cache(maxsize=None)
def tie(name):
    seed = [7, tie_names().index(name)]
    if name == DENSE:
        layout = {0: np.arange(8192, 8192 + 64), 1: _spread(100, 5, BLOCK, 101)}
        return _tie_case(TIE_N, layout, 30, None, 500, seed)
    counts, need, neg = TIE_TABLE[name]
    return _tie_case(TIE_N, _three(*counts), need, neg, 500, seed)


# ---- long cases: more than 64 blocks -------------------------------------------
LONG_N = 66 * BLOCK + 3          # 67 blocks: the second trip of the per-tensor block loops
LONG_TABLE = {                   # 50 ties in each of blocks 0, 63, 64, 65
    "cut64_neg_kept": (120, 110),
    "cut64_neg_dropped": (120, 130),
    "cut65_neg_kept": (170, 149),
}


def long_names():
    return list(LONG_TABLE)


@functools.lru_cache(maxsize=None)
def long(name):
    need, neg = LONG_TABLE[name]
    layout = {b: _spread(50, 3 + b, BLOCK, 1201) for b in (0, 63, 64, 65)}
    x, k, facts = _tie_case(LONG_N, layout, need, neg, 10_000 - need, [11, long_names().index(name)])
    assert facts["neg_block"] == 64
    return x, k, facts


# ---- shift edges: tie-free, the kept minimum on each side of the +1e-7 rule -----
EDGE_N, EDGE_K = 777, 100
_P1EM7 = int(F1EM7.view(np.uint32))
EDGE_TABLE = {                   # name -> (pattern of the kept minimum, negative?, others negative?)
    "min_1em7": (_P1EM7, False, False),                        # float32(1e-7) < 1e-7 is false: no shift
    "min_below_1em7": (_P1EM7 - 1, False, False),              # nextafter(float32(1e-7), 0): shift
    "min_minus_1em7": (_P1EM7, True, False),                   # shift; that element becomes exactly 0.0
    "all_negative": (0x3F800000, True, True),
}
EDGE_DENORMAL = "min_denormal"   # 1e-45 = pattern 1: only 0.0 lies below it


def edge_names():
    return list(EDGE_TABLE) + [EDGE_DENORMAL]


@functools.lru_cache(maxsize=None)
def edge(name):
    rng = np.random.default_rng([13, edge_names().index(name)])
    if name == EDGE_DENORMAL:
        pats = np.concatenate([[0, 1], 0x3F800000 + 4096 * np.arange(1, EDGE_N - 1)]).astype(np.uint32)
        x = rng.permutation(pats).view(np.float32)              # all positive, the zero is dropped
        return _freeze(x), EDGE_N - 1, {"kept_min": np.float32(1e-45), "shifted": True, "n_zero": 0}
    pmin, neg_min, neg_rest = EDGE_TABLE[name]
    top = (pmin + 4096 * np.arange(1, EDGE_K) + 0x01000000).astype(np.uint32)      # the other kept magnitudes
    low = (pmin - 1 - 1024 * np.arange(1, EDGE_N - EDGE_K + 1)).astype(np.uint32)  # dropped: distinct, smaller
    assert low.min() > 0 and top.max() < MAXP
    neg = np.uint32(0x80000000)
    vals = np.concatenate([[np.uint32(pmin) | (neg if neg_min else np.uint32(0))],
                           top | (neg if neg_rest else np.uint32(0)),
                           low | (rng.integers(0, 2, low.size, dtype=np.uint32) << np.uint32(31))])
    x = rng.permutation(vals).view(np.float32)
    kmin = (np.uint32(top.max()) | neg).view(np.float32) if neg_rest else vals[:1].view(np.float32)[0]
    shifted = bool(neg_min or neg_rest or pmin < _P1EM7)
    return _freeze(x), EDGE_K, {"kept_min": np.float32(kmin), "shifted": shifted,
                                "n_zero": int(name == "min_minus_1em7")}


# ---- zero threshold: k exceeds the non-zero count -------------------------------
ZERO_N = BLOCK + 500
ZERO_TABLE = {"cut_b0": 300, "cut_b1": BLOCK + 100, "all": ZERO_N - 100}    # zeros kept


def zero_names():
    return list(ZERO_TABLE)


@functools.lru_cache(maxsize=None)
def zero(name):
    """100 positive values >= 1, every other element +0.0 or -0.0 at random:
    the kept zeros are the lowest-index ones, become +1e-7 and count positive."""
    rng = np.random.default_rng([17, zero_names().index(name)])
    x = (rng.integers(0, 2, ZERO_N, dtype=np.uint32) << np.uint32(31)).view(np.float32).copy()
    nz = rng.choice(ZERO_N, 100, replace=False)
    x[nz] = np.float32(1.0) + np.arange(100, dtype=np.float32) / np.float32(128)
    need = ZERO_TABLE[name]
    zero_idx = np.setdiff1d(np.arange(ZERO_N), nz)
    return _freeze(x), 100 + need, {"T": 0, "need": need, "kept_zeros": zero_idx[:need], "shifted": True,
                                    "n_pos": 100 + need}


# ---- infinities: surely kept, abs_sum = inf -------------------------------------
INF_N = 5000


def inf_names():
    return ["mixed", "positive"]


@functools.lru_cache(maxsize=None)
def inf(name):
    rng = np.random.default_rng([19, inf_names().index(name)])
    pats = np.unique(rng.integers(0x30000000, 0x50000000, INF_N + 64))[:INF_N]
    x = _from_patterns(pats, rng).copy()
    if name == "positive":                                      # every kept value positive: no shift
        x = np.abs(x)
    at = rng.choice(INF_N, 5, replace=False)
    x[at] = np.array([np.inf, -np.inf, np.inf, -np.inf, np.inf] if name == "mixed" else [np.inf] * 5, np.float32)
    return _freeze(x), 50, {"shifted": name == "mixed", "n_inf": 5}


# ---- p = 1.0: k = n, a ternary class absent -------------------------------------
FULL_N = 3000


def full_names():
    return ["positive", "mixed", "zeros"]


@functools.lru_cache(maxsize=None)
def full(name):
    """positive: all >= 1 -> ranks {0: m}; mixed: no zeros -> {0: -m, 1: +m};
    zeros: positives and a few -float32(1e-7), which the shift turns into exact
    zeros -> {0: 0.0, 1: +m}."""
    rng = np.random.default_rng([23, full_names().index(name)])
    x = (np.float32(1.0) + rng.permutation(FULL_N).astype(np.float32) / np.float32(1024)).astype(np.float32)
    if name == "mixed":
        x *= rng.choice(np.array([-1, 1], np.float32), FULL_N)
    if name == "zeros":
        x[rng.choice(FULL_N, 7, replace=False)] = -F1EM7
    classes = {"positive": (1,), "mixed": (-1, 1), "zeros": (0, 1)}[name]
    return _freeze(x), FULL_N, {"classes": classes, "shifted": name != "positive"}


# ---- alignment batch -------------------------------------------------------------
ALIGN_SIZES = (1, 2, 3, 4, 5, 7, BLOCK - 1, BLOCK, BLOCK + 1)


def align_names():
    """(n, arena offset mod 4, k)"""
    return [(n, mod, k) for n in ALIGN_SIZES for mod in range(4) for k in sorted({1, n})]


@functools.lru_cache(maxsize=None)
def align(n, mod, k):
    rng = np.random.default_rng([29, n, mod, k])
    pats = rng.permutation(0x3A000000 + 64 * rng.permutation(1 << 17)[:n]).astype(np.uint32)   # distinct
    return _freeze(_from_patterns(pats, rng)), k, {"mod": mod}


# ---- what the fixture holds: every tie-free case the reference decides ------------
def fixture_cases():
    """-> [(id, builder, args)] of the digit, shift-edge, infinity and p = 1.0 cases."""
    out = [("digit/" + digit_id(nm), digit, nm) for nm in digit_names()]
    out += [("edge/" + nm, edge, (nm,)) for nm in edge_names()]
    out += [("inf/" + nm, inf, (nm,)) for nm in inf_names()]
    out += [("full/" + nm, full, (nm,)) for nm in full_names()]
    return out


# ---- arenas ---------------------------------------------------------------------
SENTINEL = 0x7FC0BEEF            # a NaN payload no result can hold


def arena(xs, mods=None):
    """Tensors laid out in one array with gaps of 1, 2 or 3 elements (or, with
    `mods`, the gap of 1..4 that puts tensor t at an offset = mods[t] mod 4).
    -> (float32 arena, offsets, gap mask).  The gaps hold 0.0 in the input."""
    offs, acc = [], 1
    for t, x in enumerate(xs):
        if mods is not None:
            acc += (mods[t] - acc) % 4
        offs.append(acc)
        acc += x.size + (1 + t % 3 if mods is None else 1)
    a = np.zeros(acc + 4, np.float32)
    gap = np.ones(a.size, bool)
    for x, o in zip(xs, offs):
        a[o:o + x.size] = x
        gap[o:o + x.size] = False
    return a, offs, gap
