"""No GPU: the geometric-median fixture (tests/golden/make_agg_golden.py) is
what the GPU tests expect it to be, and the robust aggregators' entry points
are declared in the header and registered in the loader.

Also the host side of tests/test_gpu_aggregation_counts.py: the 0/1 proof of
the register median's exchange lists (tests/median_net_host.cpp), the designed
median columns for any collaborator count, the inputs of the single-element
weighted average with the proof that they tell summation orders apart, and a
float64 NumPy restatement of the geometric median shown equal to the
reference on every fixture case."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from tests import agg_golden, golden_io

CASES = {  # name: (collaborators, shape, rounds asserted by the GPU test)
    "c5_shift": (5, (37, 29), True),
    "c3_small_scale": (3, (1000,), True),
    "c3_chunks": (3, (12293,), True),
    "c16_outlier": (16, (2049,), True),
    "c2_equal_513": (2, (513,), True),
    "c2_equal_1": (2, (1,), True),
    "c1_single": (1, (4097,), True),
    "c3_identical": (3, (300,), False),
}
NEW_SYMBOLS = ("ofl_median_delta", "ofl_gmedian_workspace_bytes", "ofl_gmedian_delta", "ofl_agg_delta_seeds")


def test_golden_file_shapes_and_dtypes():
    arrays, index = agg_golden.load()
    assert os.path.getsize(os.path.join(golden_io.GOLDEN, "geometric_median_golden.npz")) <= 256 * 1024
    assert {c["name"] for c in index["cases"]} == set(CASES)
    assert (index["maxiter"], index["eps"], index["ftol"]) == (4, 1e-5, 1e-6)
    for c in index["cases"]:
        C, shape, asserted = CASES[c["name"]]
        assert (c["C"], tuple(c["shape"]), c["assert_rounds"]) == (C, shape, asserted)
        q = arrays["q_" + c["name"]]
        assert q.dtype == np.int8 and q.shape == (C,) + shape
        assert arrays["mul_" + c["name"]].dtype == np.float32 and arrays["mul_" + c["name"]].shape == (C,)
        assert arrays["add_" + c["name"]].dtype == np.float32 and arrays["add_" + c["name"]].shape == (C,)
        w = arrays["w_" + c["name"]]
        assert w.dtype == np.float64 and w.shape == (C,) and w.sum() > 0
        ref = arrays["ref_" + c["name"]]
        assert ref.dtype == np.float64 and ref.shape == shape and np.isfinite(ref).all()
        xs = agg_golden.inputs(arrays, c["name"])
        assert len(xs) == C and all(x.dtype == np.float32 and x.shape == shape for x in xs)
        assert 1 <= c["rounds"] <= 4 and len(c["objectives"]) == c["rounds"] + 1


def test_golden_rounds_are_decided_with_margin():
    """Wherever a round count is asserted, |prev - obj| / (ftol * obj) is at
    least a decade away from 1 at every round (null: obj == 0, never breaks),
    and the recorded decisions are the reference's: a break ends the rounds."""
    _, index = agg_golden.load()
    for c in index["cases"]:
        objs, ratios = c["objectives"], c["ratios"]
        assert len(ratios) == c["rounds"]
        for k, (prev, obj, r) in enumerate(zip(objs, objs[1:], ratios)):
            if r is None:
                assert obj == 0
                continue
            assert r == pytest.approx(abs(prev - obj) / (index["ftol"] * obj))
            if c["assert_rounds"]:
                assert r <= 0.1 or r >= 10, (c["name"], k, r)
                if r < 1:  # a break: the last round recorded
                    assert k == c["rounds"] - 1, (c["name"], k)
                elif k == c["rounds"] - 1:  # no break on the last round: maxiter ran out
                    assert c["rounds"] == index["maxiter"], c["name"]
    rounds = {c["name"]: c["rounds"] for c in index["cases"]}
    assert rounds["c2_equal_513"] == rounds["c2_equal_1"] == 1  # equal weights: stops after the first round
    assert rounds["c1_single"] == 4                            # obj == 0 never breaks


def test_new_symbols_in_header_and_loader():
    from openfl_amd import _lib
    with open(os.path.join(golden_io.GOLDEN, "..", "..", "include", "ofl_codec.h")) as f:
        declared = set(re.findall(r"\b(ofl_[a-z0-9_]+)\s*\(", f.read()))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name


def test_aggregation_names_and_collaborator_limits():
    from openfl_amd import aggregation
    assert aggregation.AGGREGATIONS == ("weighted_average", "median", "geometric_median")
    assert aggregation._MEDIAN_MAX_C == 128 and aggregation._GMEDIAN_MAX_C == 16


# ------------------------------------ register median: the 0/1 proof, host ---
ROOT = os.path.normpath(os.path.join(golden_io.GOLDEN, "..", ".."))
MEDIAN_REGISTER_C = tuple(range(1, 17))              # one compare-exchange network each
MEDIAN_LDS_C = (17, 18, 31, 32, 64, 65, 127, 128)    # the LDS insertion sort


def zero_one_columns(C):
    """The (C, 2^C) float32 stack whose column m holds the bits of m."""
    m = np.arange(1 << C, dtype=np.uint32)
    return np.stack([((m >> c) & 1).astype(np.float32) for c in range(C)])


def _cxx17():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    return None


def test_median_network_zero_one_proof_on_the_host(tmp_path):
    """median_net.h compiled for the host: every 0/1 column of every C = 1..16
    against std::sort (tests/median_net_host.cpp).  A compare-exchange network
    that is right on all 0/1 inputs is right on all NaN-free inputs, so this
    pins make_net's exchange lists without a GPU.  The exchange counts of the
    powers of two are Batcher's (1, 5, 19, 63), and dropping the exchanges
    with a padding slot never adds one."""
    cxx = _cxx17()
    if cxx is None:
        pytest.skip("no C++17 compiler (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "median_net_host")
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "openfl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "median_net_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    rows = re.findall(r"^C (\d+) exchanges (\d+) columns (\d+) mismatches (\d+)$", run.stdout, re.M)
    assert [int(r[0]) for r in rows] == list(MEDIAN_REGISTER_C), run.stdout
    assert all(int(r[2]) == 1 << int(r[0]) and int(r[3]) == 0 for r in rows), run.stdout
    assert run.returncode == 0
    exchanges = {int(r[0]): int(r[1]) for r in rows}
    assert (exchanges[1], exchanges[2], exchanges[4], exchanges[8], exchanges[16]) == (0, 1, 5, 19, 63)
    assert all(exchanges[c] < exchanges[c + 1] for c in range(1, 16))


def test_zero_one_columns():
    for C in (1, 2, 5, 16):
        s = zero_one_columns(C)
        assert s.dtype == np.float32 and s.shape == (C, 1 << C)
        assert np.array_equal(np.unique(s), [0.0, 1.0])
        assert len({tuple(col) for col in s.T.tolist()}) == 1 << C      # every column once
        assert set(np.unique(np.median(s, axis=0)).tolist()) <= {0.0, 0.5, 1.0}


# ----------------------------------------------- designed median columns ---
def designed_columns(C):
    """-> (stack (C, columns) float32, one label per column).  The columns of
    test_median_designed_columns for any collaborator count: all-equal,
    two-value duplicates that straddle the middle, ramps, +-inf mixtures,
    3e38 at both middle ranks (even C: the float32 sum overflows), subnormals
    whose middle pair sums to an odd number of units, +-0 ties, a NaN in every
    row position among finite values and among infinities, all NaN.  Values
    given in rank order are also placed by a fixed permutation of the rows."""
    inf, nan = np.inf, np.nan
    h, r = C // 2, np.arange(C)
    perm = np.random.default_rng(C).permutation(C)
    cols, labels = [], []

    def add(label, c, shuffled=False):
        c = np.asarray(c, np.float32)
        assert c.shape == (C,), label
        cols.append(c)
        labels.append(label)
        if shuffled:
            cols.append(c[perm])
            labels.append(label + "/shuffled")

    add("equal", np.full(C, 7.0))
    add("equal-negative", np.full(C, -1.5))
    add("straddle", [1.0] * h + [2.0] * (C - h), shuffled=True)
    add("straddle-low-majority", [1.0] * (C - h) + [2.0] * h, shuffled=True)
    add("straddle-alternating", np.where(r % 2, 1.0, 2.0))
    add("ascending", r)
    add("descending", r[::-1], shuffled=True)
    add("all+inf", np.full(C, inf))
    add("all-inf", np.full(C, -inf))
    add("inf-thirds", np.where(r % 3 == 0, inf, np.where(r % 3 == 1, -inf, r)))
    c = r.astype(np.float64)
    c[0], c[-1] = inf, -inf
    add("inf-ends", c)
    add("inf-halves", [-inf] * h + [inf] * (C - h), shuffled=True)   # even C: mean(-inf, inf) is NaN
    c = np.full(C, inf)
    c[:min(2, C)] = [1.0, 2.0][:min(2, C)]
    add("inf-majority", c, shuffled=True)
    lows, two = max(h - 1, 0), min(2, C)
    big = [1.0] * lows + [3e38] * two + [3.3e38] * (C - lows - two)  # even C: ranks C/2 - 1 and C/2 hold 3e38
    add("overflow", big, shuffled=True)
    add("overflow-negative", -np.asarray(big), shuffled=True)
    sub = [1e-45] * h + [3e-45] * (C - h)                            # 1 and 2 units: the middle pair sums to 3
    add("subnormal", sub, shuffled=True)
    add("subnormal-negative", -np.asarray(sub), shuffled=True)
    add("zeros-alternating", np.where(r % 2, -0.0, 0.0))
    add("zeros-halves", [-0.0] * h + [0.0] * (C - h), shuffled=True)
    c = np.where(r % 2, 0.0, -0.0)
    c[0], c[-1] = -1.0, 1.0
    add("zeros-between", c)
    for row in range(C):
        c = r.astype(np.float64)
        c[row] = nan
        add(f"nan-row{row}-finite", c)
        c = np.where(r % 2, -inf, inf)
        c[row] = nan
        add(f"nan-row{row}-infinite", c)
    add("all-nan", np.full(C, nan))
    return np.stack(cols, axis=1), labels


def designed_stack(C):
    """The designed columns laid out twice, forward and reversed, so that both
    the 16-byte body and the scalar tail of a kernel see every one."""
    stack, labels = designed_columns(C)
    return np.ascontiguousarray(np.concatenate([stack, stack[:, ::-1]], axis=1)), labels + labels[::-1]


def median_reference(stack):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return np.median(stack, axis=0)


def assert_designed_reference(C, stack, ref):
    """The design has not degenerated: the reference holds a NaN for every NaN
    column and both infinities; for even C the overflow columns are finite
    going in and infinite coming out."""
    assert ref.dtype == np.float32 and ref.shape == (stack.shape[1],)
    assert np.isnan(ref).sum() >= 2 * (2 * C + 1), C
    assert np.isposinf(ref).any() and np.isneginf(ref).any(), C
    if C % 2 == 0:
        over = np.isfinite(stack).all(axis=0) & np.isinf(ref)
        assert over.sum() >= 8 and np.isposinf(ref[over]).any() and np.isneginf(ref[over]).any(), C


@pytest.mark.parametrize("C", MEDIAN_REGISTER_C + MEDIAN_LDS_C)
def test_designed_columns_hold_the_design(C):
    stack, labels = designed_stack(C)
    assert stack.dtype == np.float32 and stack.shape == (C, len(labels))
    assert stack.shape[1] == 62 + 4 * C                       # never a multiple of 4: a body and a tail
    ref = median_reference(stack)
    assert_designed_reference(C, stack, ref)
    by = {lab: ref[k] for k, lab in enumerate(labels[:len(labels) // 2])}
    assert all(np.isnan(by[f"nan-row{row}-{kind}"]) for row in range(C) for kind in ("finite", "infinite"))
    assert np.isnan(by["all-nan"]) and by["all+inf"] == np.inf and by["all-inf"] == -np.inf
    assert by["equal"] == 7.0 and by["ascending"] == by["descending"] == by["descending/shuffled"] == (C - 1) / 2
    assert by["zeros-alternating"] == 0.0 and by["zeros-halves"] == 0.0
    if C % 2 == 0:
        assert by["straddle"] == by["straddle/shuffled"] == 1.5
        assert by["overflow"] == by["overflow/shuffled"] == np.inf
        assert by["overflow-negative"] == -np.inf
        assert np.isnan(by["inf-halves"])
        # 1.5 units of the smallest subnormal round to even, as NumPy's division does
        assert by["subnormal"].tobytes() == np.float32(3e-45).tobytes()
        assert by["subnormal-negative"].tobytes() == np.float32(-3e-45).tobytes()
    else:
        assert by["straddle"] == 2.0 and by["straddle-low-majority"] == 1.0
        assert by["subnormal"].tobytes() == np.float32(3e-45).tobytes()


# ------------------- single-element weighted average: inputs and their power ---
WAVG_POINT_C = (7, 8, 9, 15, 16, 17, 127, 128, 129, 130, 136, 137, 255, 256, 257, 264, 1000, 2047, 2048)
WAVG_POINTS = 256
_wavg_cases = {}


def _sum_in_order(p):
    s = p[0].copy()
    for c in range(1, p.shape[0]):
        s = s + p[c]
    return s


def _sum_one_block(p):
    """NumPy's unrolled block applied to all rows of p, whatever their number:
    in order below 8, else eight accumulators, their tree, then the tail."""
    n = p.shape[0]
    if n < 8:
        s = np.zeros(p.shape[1])
        for c in range(n):
            s = s + p[c]
        return s
    r = [p[k].copy() for k in range(8)]
    k = 8
    while k < n - n % 8:
        for j in range(8):
            r[j] = r[j] + p[k + j]
        k += 8
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for c in range(k, n):
        s = s + p[c]
    return s


def _sum_pairwise(p):
    """NumPy's pairwise sum of the rows of p: one block up to 128 rows, else
    halves, the first rounded down to a multiple of 8."""
    n = p.shape[0]
    if n <= 128:
        return _sum_one_block(p)
    n2 = n // 2
    n2 -= n2 % 8
    return _sum_pairwise(p[:n2]) + _sum_pairwise(p[n2:])


def wavg_point_case(C):
    """256 single-element tensors per collaborator (one arena of 256 float32
    each, magnitudes spread over 1e-3..1e3 per collaborator), weights
    rng.random(C) * 5 and a base.  The reference of column j is np.average of
    the (C, 1) stack.  Also the fraction of columns on which two other
    summation orders give other bits; computed once, from the inputs alone."""
    if C in _wavg_cases:
        return _wavg_cases[C]
    rng = np.random.default_rng(9000 + C)
    x = np.stack([(rng.standard_normal(WAVG_POINTS) * 10.0 ** rng.integers(-3, 3)).astype(np.float32)
                  for _ in range(C)])
    w = rng.random(C) * 5
    base = rng.standard_normal(WAVG_POINTS).astype(np.float32)
    avg = np.empty(WAVG_POINTS)
    for j in range(WAVG_POINTS):
        avg[j] = np.average(x[:, j:j + 1], weights=w, axis=0)[0]
    wsum = np.average(x[:, :1], weights=w, axis=0, returned=True)[1][0]
    p = x.astype(np.float64) * w[:, None]
    differs = lambda s: float(np.mean((s / wsum).view(np.uint64) != avg.view(np.uint64)))  # noqa: E731
    case = dict(x=x, w=w, base=base, avg=avg, wsum=float(wsum), delta64=avg - base.astype(np.float64),
                in_order_differs=differs(_sum_in_order(p)), one_block_differs=differs(_sum_one_block(p)),
                pairwise_differs=differs(_sum_pairwise(p)))
    case["delta32"] = case["delta64"].astype(np.float32)
    _wavg_cases[C] = case
    return case


def assert_wavg_points_discriminate(C, case):
    """The inputs can tell the summation orders apart: from 16 collaborators
    on at least a quarter of the columns differ in bits from the in-order
    sum, and above 128 at least a quarter differ from one unsplit block."""
    if C >= 16:
        assert case["in_order_differs"] >= 0.25, (C, case["in_order_differs"])
    if C > 128:
        assert case["one_block_differs"] >= 0.25, (C, case["one_block_differs"])


@pytest.mark.parametrize("C", WAVG_POINT_C)
def test_wavg_point_inputs_tell_summation_orders_apart(C):
    case = wavg_point_case(C)
    print(f"C={C}: differs from in-order {case['in_order_differs']:.3f}, from one block "
          f"{case['one_block_differs']:.3f}, from the pairwise restatement {case['pairwise_differs']:.3f}")
    assert case["pairwise_differs"] == 0.0       # the order the C ABI documents is NumPy's
    assert_wavg_points_discriminate(C, case)


# ------------------------------- geometric median: a float64 restatement ---
GM_RTOL = 1e-10


def restate_geometric_median(xs, weights, maxiter=4, eps=1e-5, ftol=1e-6):
    """ofl_gmedian_delta as include/ofl_codec.h describes it, in float64 NumPy:
    the weights divided by their sum; the median (sum_c x_c W_c) / sum(W) as
    np.average forms it; obj0 from the first average; then up to maxiter
    rounds of W <- W / max(eps, dist), renormalised, the new average, the
    objective with the new weights and the strict test |prev - obj| < ftol *
    obj.  -> (median, rounds run, objectives, stopping ratios (None: obj 0))."""
    x = np.stack([np.asarray(t, np.float32).reshape(-1) for t in xs])
    w = np.asarray(weights, np.float64)
    w = w / sum(w)

    def point(w):
        m = np.average(x, weights=w, axis=0)
        d = np.sqrt(((m[None, :] - x.astype(np.float64)) ** 2).sum(axis=1))
        return m, d, float((w * d).sum())

    m, d, obj = point(w)
    objs, ratios, rounds = [obj], [], 0
    for _ in range(maxiter):
        prev = obj
        w = w / np.maximum(eps, d)
        w = w / w.sum()
        m, d, obj = point(w)
        rounds += 1
        objs.append(obj)
        ratios.append(abs(prev - obj) / (ftol * obj) if obj != 0 else None)
        if abs(prev - obj) < ftol * obj:
            break
    return m.reshape(np.shape(xs[0])), rounds, objs, ratios


def rounds_decided(ratios):
    """The rule of test_golden_rounds_are_decided_with_margin: every stopping
    ratio at least a decade from 1 (None: obj == 0, which never stops)."""
    return all(r is None or r <= 0.1 or r >= 10 for r in ratios)


@pytest.mark.parametrize("name", sorted(CASES))
def test_geometric_median_restatement_equals_the_reference(name):
    """The restatement against the reference's recorded results, within the
    bound the GPU tests use, 1e-10 * max|x|, and with the reference's round
    count wherever the fixture asserts one.  Largest error seen over the
    eight cases: 1.0e-15 (c5_shift, bound 8.3e-10), i.e. 1.2e-16 * max|x|; the
    recorded objectives are met to 1e-9 relative."""
    arrays, index = agg_golden.load()
    case = next(c for c in index["cases"] if c["name"] == name)
    xs, w, ref = agg_golden.inputs(arrays, name), arrays["w_" + name], arrays["ref_" + name]
    got, rounds, objs, ratios = restate_geometric_median(xs, w, index["maxiter"], index["eps"], index["ftol"])
    bound = GM_RTOL * max(float(np.abs(x).max()) for x in xs)
    err = float(np.abs(got - ref).max())
    print(f"{name}: max|restated - ref| = {err:.3e}, bound {bound:.3e}, rounds {rounds} (reference {case['rounds']})")
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert err <= bound
    if case["assert_rounds"]:
        assert rounds == case["rounds"]
        assert rounds_decided(ratios)
        assert objs == pytest.approx(case["objectives"], rel=1e-9, abs=0)
