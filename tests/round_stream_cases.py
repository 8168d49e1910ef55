"""What the round-ingest and streaming-average tests share: the layout, the
pipelines and the comparisons (no device is touched on import)."""
import numpy as np

F = np.float32
DEV = "cuda:0"
# two single-element tensors and an empty one, both sides of dim_threshold
# (size == threshold included), sizes that are multiples neither of 4 (scalar
# tails) nor of 64 (gaps), and a tensor of two slices
SHAPES = [(1,), (0,), (7,), (10, 10), (101,), (3, 343), (40000,), (1,)]
DIM_THRESHOLD = 100
# the same with a tensor whose slice plan has a row-pass slice (65536 > 2^15)
SHAPES_ROW = SHAPES + [(70000,)]
# the SKC and STC pipelines' own forward refuses an empty tensor ("sparsify:
# empty batch"), per tensor and inside run() alike, so theirs has none
SHAPES_SPARSE = [s for s in SHAPES if s != (0,)]
PIPELINES = ("eden_ref", "eden_fast", "kc", "skc", "stc")


def make_pipeline(name):
    from openfl_amd import pipelines as P
    if name.startswith("eden"):
        return P.EdenPipeline(n_bits=8, dim_threshold=DIM_THRESHOLD, device=DEV,
                              seed_mode="reference" if name == "eden_ref" else "fast")
    if name == "kc":
        return P.KCPipeline(n_clusters=6, device=DEV)
    if name == "skc":
        return P.SKCPipeline(device=DEV)
    return P.STCPipeline(device=DEV)


def shapes_for(name):
    return tuple(SHAPES_SPARSE if name in ("skc", "stc") else SHAPES)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def tensors(shapes, seed, scale=0.01):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(s) * scale).astype(F) for s in shapes]


def gap_mask(re):
    inside = np.zeros(re.arena_numel, bool)
    for o, n in zip(re.offsets, re.numels):
        inside[o:o + n] = True
    return ~inside


def rng_state():
    s = np.random.get_state()
    return (s[0], s[1].tobytes(), s[2], s[3], s[4])


def md_key(mds):
    """A metadata list in a form that compares by value bits and value types."""
    out = []
    for md in mds:
        m = md.get("int_to_float")
        out.append((list(md["int_list"]) if "int_list" in md else None,
                    None if m is None else [(int(k), type(v).__name__, np.float64(v).tobytes()) for k, v in m.items()]))
    return out
