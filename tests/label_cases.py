"""Designed label records (ofl_label_rec, include/ofl_codec.h) and the numpy
reference they are compared with.  numpy only, no tests: the designs are
checked on the host by test_label_cases_cpu.py and run on the device by
test_gpu_label_designed.py -- k_label_apply (csrc/lossy_kmeans.h) through
lossy.label_apply, the TLZ encoder's lab_rank / lab_fill / lab_one
(csrc/tlz_encode.h) through lossy.gzip_ranks(x, label=), and the value records
of k_bkm_tab through lossy.kmeans_batch(value_out=).

The records' contract.  A record labels the arena elements [start, end) with
rank[c], c = the number of its seven midpoints mid[0..6] that lie below the
element in float32 comparison: a NaN takes cluster 0 and a value on a midpoint
the lower cluster.  The midpoints are non-decreasing and mid[7] = +inf; that
is what both producers (k_bkm_tab, lossy.ternary_label_table) write, and every
rule below keeps to it.  label_apply accepts empty records (start == end)
anywhere in its table.  The encoder takes non-empty, ascending,
non-overlapping records (what test_kmeans_label_table_checks enforces for
k-means output): empty records are outside its contract and are not tested
there.

Every builder is deterministic (seeded generators, no global state) and
returns read-only arrays.
"""
import functools

import numpy as np

F = np.float32
INF = F(np.inf)
FLT_MAX = np.finfo(F).max
DENORM = F(1e-45)                # the smallest denormal
CHUNK = 1 << 16                  # kBkmChunk: elements per chunk of k_label_apply
MAX_T = 4096                     # kLaMaxT: records per launch of k_label_apply
SEG = 2048                       # kSeg: values per encoder segment
MEMBER = 131072                  # kMemTok: values per gzip member
PER = 8                          # kPer: values per encoder thread
REC = np.dtype([("start", "<i8"), ("end", "<i8"), ("mid", "<f4", 8), ("rank", "<f4", 8)])
SENTINEL = 0x7B7B7B7B            # bit pattern outputs are pre-filled with (3.27e36: no rule or base gives it)


def _freeze(a):
    a.setflags(write=False)
    return a


def _f(bits):
    return np.array(bits, np.uint32).view(F)


# ---- reference ----------------------------------------------------------------
def label_index(x, mid):
    """The cluster of every element: how many of mid[:7] lie below it (float32
    comparison; every comparison with a NaN is false, so a NaN counts 0)."""
    x, m = np.asarray(x, F), np.asarray(mid, F)[:7]
    return np.sum(m[None, :] < x[:, None], axis=1).astype(np.int64)


def label_index_sorted(x, mid):
    """The same through a search of the sorted midpoints; searchsorted sorts a
    NaN behind +inf, so the NaNs are handled apart."""
    x = np.asarray(x, F)
    idx = np.searchsorted(np.asarray(mid, F)[:7], x, side="left").astype(np.int64)
    idx[np.isnan(x)] = 0
    return idx


def label_values(x, rec, index=label_index):
    return np.asarray(rec["rank"], F)[index(x, rec["mid"])]


def applied(x, recs, base, index=label_index):
    """label_apply in plain numpy: -> (out as float32 with SENTINEL outside the
    records, inside mask).  out = base + value in float32, the value itself
    without a base."""
    out = np.full(x.size, SENTINEL, np.uint32).view(F)
    inside = np.zeros(x.size, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in recs:
            s, e = int(r["start"]), int(r["end"])
            if e <= s:
                continue
            d = label_values(x[s:e], r, index)
            out[s:e] = d if base is None else (base[s:e] + d).astype(F)
            inside[s:e] = True
    return out, inside


def ranks_of(x, recs, index=label_index):
    """The rank array the fused encoder labels: 0 outside the records."""
    out = np.zeros(x.size, F)
    for r in recs:
        s, e = int(r["start"]), int(r["end"])
        out[s:e] = label_values(x[s:e], r, index)
    return out


def same_bits(got, want):
    """Bit for bit as uint32, NaN positions as a mask (x86 and the GPU differ
    in the sign of the default NaN): -> number of elements that differ."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    gn, wn = np.isnan(got), np.isnan(want)
    return int(np.sum(gn != wn) + np.sum((got.view(np.uint32) != want.view(np.uint32)) & ~wn & ~gn))


# ---- rules ----------------------------------------------------------------------
def _mids(*finite):
    m = np.full(8, INF, F)
    m[:len(finite)] = finite
    assert np.all(m[1:] >= m[:-1]) and m[7] == INF
    return _freeze(m)


_LADDER = (-2.5, -0.75, -0.125, 0.375, 1.25, 6.5, 1000.0)
RULES = {"k1": _mids()}
RULES.update({f"k{k}": _mids(*_LADDER[:k - 1]) for k in range(2, 9)})
RULES.update({
    "dup2": _mids(-1.5, 0.5, 0.5, 2.25),                         # three equal centres of a fit with nuniq < k
    "dup3": _mids(-1.5, 0.5, 0.5, 0.5, 2.25, 2.25),
    "ternary": _mids(-DENORM, 0.0),                              # lossy.ternary_label_table
    "fltmax": _mids(-FLT_MAX, -1.0, FLT_MAX),
    "denormal": _mids(_f(0x80000003), _f(0x00000002), _f(0x007FFFFF), np.finfo(F).tiny, 1.0),
})
RULE_NAMES = tuple(RULES)

# values of label_apply's records: non-integers, both zeros, both infinities, a
# denormal, and adjacent clusters with one value
VALUE_SETS = tuple(_freeze(np.array(v, F)) for v in (
    (-3.75, 0.1, 2.5e-3, -0.0, 0.0, 1.5, 7.25, -100.125),
    (np.inf, -np.inf, 3e-45, 0.3, 0.3, -0.0, 1e30, -2.5),
    (-0.0, 0.0, -1e-40, 11.5, -np.inf, 0.625, 0.625, np.inf),
))
# ranks of the encoder's records: integers 0..31 out of order, 31, a repeated rank
RANK_SETS = tuple(_freeze(np.array(v, F)) for v in (
    (5, 31, 7, 17, 5, 2, 30, 0),                     # 0, what a gap gives, only in the cluster few rules reach
    (9, 3, 31, 4, 4, 12, 1, 20),
))
GAP_FILL = _freeze(np.array([np.nan, np.inf, 32.0, 2.5], F))    # what lies between the encoder's records


def reachable(mid):
    """The clusters some value can take: 0 (a NaN, -inf), and c where
    mid[c - 1] < mid[c], the values of (mid[c - 1], mid[c]]."""
    m = np.asarray(mid, F)
    return {0} | {c for c in range(1, 8) if m[c - 1] < m[c]}


PATTERN = 61                     # a rule's probes and filler: any 61 consecutive elements of a record hold them all


@functools.lru_cache(maxsize=None)
def probes(rule):
    """Every finite midpoint with its float32 neighbours, +-0, +-1e-45,
    +-FLT_MAX, +-inf, NaN of both signs."""
    m = RULES[rule]
    fin = m[np.isfinite(m)]
    with np.errstate(over="ignore"):             # FLT_MAX's neighbour is inf
        near = [np.nextafter(fin, INF), np.nextafter(fin, -INF)]
    p = [fin] + near + [np.array([0.0, -0.0, DENORM, -DENORM, FLT_MAX, -FLT_MAX, np.inf, -np.inf], F),
                        _f([0x7FC00000, 0xFFC00000])]
    return _freeze(np.concatenate(p).astype(F))


@functools.lru_cache(maxsize=None)
def pattern(rule):
    """The rule's probes, shuffled with filler drawn around its midpoints, PATTERN values."""
    rng = np.random.default_rng([7, RULE_NAMES.index(rule)])
    p = probes(rule)
    fill = (rng.standard_normal(PATTERN - p.size) * rng.choice([0.3, 3.0, 2000.0], PATTERN - p.size)).astype(F)
    return _freeze(rng.permutation(np.concatenate([p, fill])))


def record_values(rule, t, n):
    """The n elements of record number t: its rule's pattern from a phase that moves with t."""
    return pattern(rule)[(17 * t + np.arange(n)) % PATTERN]


# ---- layouts of label_apply -----------------------------------------------------
COUNTS = (1, 63, 64, 65, 127, 4095, 4096, 4097, 4160)
EMPTY_KINDS = ("first", "last", "middle", "run70", "around4096", "only")
APPLY_LAYOUTS = ("short", "chunks") + tuple(f"counts/{n}" for n in COUNTS) + tuple(f"empty/{k}" for k in EMPTY_KINDS)
SHORT_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9)
CHUNK_LENGTHS = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)


def placed(specs, lead=0, tail=3):
    """specs: (length, start mod 4 or None, gap before) -> starts, ends, arena length."""
    starts, ends, at = [], [], lead
    for n, mod, gap in specs:
        at += gap
        while mod is not None and at % 4 != mod:
            at += 1
        starts.append(at)
        ends.append(at + n)
        at += n
    return _freeze(np.array(starts, np.int64)), _freeze(np.array(ends, np.int64)), at + tail


def _counts_specs(n, seed):
    rng = np.random.default_rng([11, seed])
    return [(int(a), None, int(g)) for a, g in zip(rng.integers(1, 6, n), rng.integers(0, 4, n))]


@functools.lru_cache(maxsize=None)
def apply_layout(name):
    """-> (starts, ends, arena length)."""
    kind, _, arg = name.partition("/")
    if kind == "short":       # every length below, at and above the peel, at every alignment
        return placed([(n, mod, 1) for mod in range(4) for n in SHORT_LENGTHS], lead=4)
    if kind == "chunks":      # one chunk less one, one, one and one element, two and five elements
        return placed([(n, mod, 2) for mod in (0, 1) for n in CHUNK_LENGTHS])
    if kind == "counts":
        return placed(_counts_specs(int(arg), int(arg)), lead=2)
    assert kind == "empty"
    nt = {"around4096": 4200, "only": 5}.get(arg, 300)
    specs = _counts_specs(nt, 90 + EMPTY_KINDS.index(arg))
    empty = {"first": [0], "last": [nt - 1], "middle": [nt // 2], "run70": range(100, 170),
             "around4096": [4095, 4096], "only": range(nt)}[arg]
    for t in empty:
        specs[t] = (0, None, specs[t][2])
    return placed(specs, lead=1)


def record_rule(t, rot):
    """Record t's (rule name, value / rank set number): neighbours differ, and rot moves both."""
    return RULE_NAMES[(t + rot) % len(RULE_NAMES)], (t // len(RULE_NAMES) + t + rot)


def _records(starts, ends, rot, sets):
    recs = np.zeros(len(starts), REC)
    recs["start"], recs["end"] = starts, ends
    for t in range(len(starts)):
        rule, s = record_rule(t, rot)
        recs["mid"][t], recs["rank"][t] = RULES[rule], sets[s % len(sets)]
    return recs


def _fill(x, recs, rot):
    for t, r in enumerate(recs):
        x[r["start"]:r["end"]] = record_values(record_rule(t, rot)[0], t, int(r["end"] - r["start"]))


@functools.lru_cache(maxsize=None)
def apply_case(name, rot=0):
    """-> (x arena, records, base arena): gaps of x hold GAP_FILL, the base a
    few -0.0 and infinities among ordinary values."""
    starts, ends, n = apply_layout(name)
    assert n < 1_000_000
    recs = _records(starts, ends, rot, VALUE_SETS)
    x = GAP_FILL[np.arange(n) % 4].copy()
    _fill(x, recs, rot)
    base = (np.random.default_rng([13, APPLY_LAYOUTS.index(name)]).standard_normal(n) * 0.1).astype(F)
    base[::97], base[5::1013], base[7::1019] = -0.0, -np.inf, np.inf
    return _freeze(x), _freeze(recs), _freeze(base)


def chunk_counts(recs):
    n = recs["end"] - recs["start"]
    return (n + CHUNK - 1) // CHUNK


# ---- layouts of the encoder -------------------------------------------------------
EDGES = (SEG - 1, SEG, SEG + 1, MEMBER - 1, MEMBER, MEMBER + 1)
EDGE_VARIANTS = ("adjacent", "end", "begin")
WINDOWS = (5, 6, 64, 300)
ENCODER_LAYOUTS = tuple(f"edges/{b}/{v}" for b in EDGES for v in EDGE_VARIANTS) + ("edges/span3",) + \
    tuple(f"window/{n}" for n in WINDOWS) + ("octet", "single")
OCTET_AT = (64, 2 * SEG + 40)    # the aligned groups of 8 values of the octet layout
OCTET_CUTS = (0, 1, 3, 4, 5, 7, 8)


def window_segment(n):
    """The segment the window layout's n short records lie in."""
    return 0 if n in (5, 64) else 1


@functools.lru_cache(maxsize=None)
def encoder_layout(name):
    """-> (starts, ends, arena length): non-empty ascending records, a gap before the first and after the last."""
    kind, _, arg = name.partition("/")
    if kind == "edges" and arg == "span3":          # begins in member 0, covers member 1, ends in member 2
        s = np.array([7, MEMBER - 100], np.int64)
        e = np.array([300, 2 * MEMBER + 77], np.int64)
        return _freeze(s), _freeze(e), 2 * MEMBER + 77 + 9
    if kind == "edges":
        b, variant = int(arg.split("/")[0]), arg.split("/")[1]
        pairs = {"adjacent": [(b - 900, b), (b, b + 900)],
                 "end": [(b - 900, b), (b + 2, b + 600)],
                 "begin": [(b - 900, b - 2), (b, b + 900)]}[variant]
        s, e = np.array(pairs, np.int64).T
        return _freeze(s.copy()), _freeze(e.copy()), b + 900 + 5
    if kind == "window":
        n = int(arg)
        rng = np.random.default_rng([17, n])
        specs = [(int(a), None, int(g)) for a, g in zip(rng.integers(1, 7, n), rng.integers(0, 3, n))]
        s, e, end = placed(specs, lead=window_segment(n) * SEG + 3, tail=0)
        nxt = (window_segment(n) + 1) * SEG
        assert end <= nxt
        s, e = np.append(s, nxt + 10), np.append(e, nxt + 10 + 3000)
        return _freeze(s), _freeze(e), nxt + 10 + 3000 + 6
    if kind == "octet":
        s, e = [3], [40]
        for at in OCTET_AT:
            s += [at + c for c in OCTET_CUTS[:-1]]
            e += [at + c for c in OCTET_CUTS[1:]]
        s, e = s + [OCTET_AT[1] + 11], e + [OCTET_AT[1] + 500]
        return _freeze(np.array(s, np.int64)), _freeze(np.array(e, np.int64)), e[-1] + 4
    assert kind == "single"
    return _freeze(np.array([5], np.int64)), _freeze(np.array([5000], np.int64)), 6000


@functools.lru_cache(maxsize=None)
def encoder_case(name, one_off=False):
    """-> (x arena, records).  one_off: the arena without its first element
    (a gap), every record one position lower -- handed over as a view one
    element into an aligned allocation it takes the encoder's unaligned loads."""
    starts, ends, n = encoder_layout(name)
    assert starts[0] >= 1 and ends[-1] < n and np.all(starts[1:] >= ends[:-1]) and np.all(ends > starts)
    recs = _records(starts, ends, ENCODER_LAYOUTS.index(name), RANK_SETS)
    x = GAP_FILL[np.arange(n) % 4].copy()
    _fill(x, recs, ENCODER_LAYOUTS.index(name))
    if one_off:
        x = x[1:].copy()
        recs["start"] -= 1
        recs["end"] -= 1
    return _freeze(x), _freeze(recs)


def refused_case(bad):
    """The single layout with one rank replaced by `bad` in a cluster an element takes: -> (x, records)."""
    x, recs = encoder_case("single")
    recs = recs.copy()
    c = int(label_index(x[5:6], recs["mid"][0])[0])
    recs["rank"][0][c] = bad
    return x, _freeze(recs)


# ---- chain tensors: the value records of k_bkm_tab ---------------------------------
CHAIN_K = 6
CHAIN_REPEAT = 40
# at most CHAIN_K distinct values, so a fit returns exactly them as uniq
# (ascending, as np.unique gives them).  The map of the backward is {i: uniq[i]}.
CHAINS = {
    "full": (1.0, 2.0, 3.0, 4.0, 5.0, 9.0),          # rank 0 -> 1 -> 2 -> 3 -> 4 -> 5 -> 9
    "partial": (1.0, 2.0, 2.5, 7.0, 8.0, 9.5),       # rank 0 -> 1 -> 2 -> 2.5 and no further
    "earlier": (-0.5, 0.0, 1.0, 2.0, 3.0, 3.5),      # values equal to EARLIER keys: not replaced again
    "none": (0.25, 0.75, 1.5, 6.5, 7.25, 8.5),       # no value is a key
    "fewer": (1.0, 2.0, 7.5),                        # fewer distinct values than k: 0 -> 1 -> 2 -> 7.5
}
CHAIN_NAMES = tuple(CHAINS)


@functools.lru_cache(maxsize=None)
def chain_tensor(name):
    v = np.array(CHAINS[name], F)
    return _freeze(np.random.default_rng([19, CHAIN_NAMES.index(name)]).permutation(np.repeat(v, CHAIN_REPEAT)))


def chain_ref(ranks, uniq):
    """The reference's backward, literally (kc_pipeline.py:79-83), on a float32 rank array."""
    data = np.array(ranks, F)
    int2float_map = {i: u for i, u in enumerate(uniq)}
    for key in int2float_map:
        indices = data == key
        data[indices] = int2float_map[key]
    return data


def chain_until_stable(ranks, uniq):
    """What the backward is NOT: the loop repeated until nothing changes."""
    data = np.array(ranks, F)
    while True:
        nxt = chain_ref(data, uniq)
        if np.array_equal(nxt, data):
            return data
        data = nxt
