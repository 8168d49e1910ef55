"""The large-slice schedule variants that tests/test_gpu_eden_variants.py runs
and that the coverage ledger in tests/test_seed_and_abi.py checks on the host
(plan creation needs no GPU): one list, so the ledger speaks about exactly the
plans the GPU test executes.

A 5-pass slice splits into MALL sub-waves (explicit tile lists) only from 2^26
elements, so that is the shape."""

# Tensor 0: one 2^26 slice whose valid length ends inside a float4 and leaves
# whole row tiles without input.  Tensor 1: dims [2^26, 8], so every plane row
# is 2^23 + 1 bytes long: the byte-wise plane path of k_dec_rowA2<false>, under
# explicit tile lists in the split configs.  Tensor 2: one small slice.
NUMELS = [(1 << 26) - 99_997, (1 << 26) + 7, 3000]

# (row2, pair, wave_mib) as EdenPlan takes them; None: the library's default
# plan (128 MiB waves on two streams, everything auto -- the schedule that
# test_five_pass_slices_vs_oracle[2^26] ties to the oracle), which goes first
# and is the one every other config is compared with.  The other plans run on
# one stream.
VARIANT_CONFIGS = [
    None,
    (0, 0, 4096),     # persistent row kernels, whole-slice passes, one wave
    (0, -1, 64),      # persistent, whole-slice passes, each 2^26 slice a wave of its own (no split: row2 = 0)
    (-1, 0, 64),      # split into sub-waves, unpaired explicit tile lists
    (-1, 1, 64),      # split, paired explicit tile lists
    (1, 1, 4096),     # two blocks per CU over the whole wave, paired table
    (1, 0, 4096),     # ... unpaired (not split: the wave holds the slices)
]


def make_plan(cfg, numels=NUMELS, n_bits=8):
    from openfl_amd.codec import EdenPlan
    if cfg is None:
        return EdenPlan(numels, n_bits)
    row2, pair, wave = cfg
    return EdenPlan(numels, n_bits, wave_mib=wave, streams=1, row2=row2, pair=pair)


def row_launches(plan):
    """{(direction, kernel name, expl, paired)} over the plan's row launches
    (kernel names without the ofl:: prefix and template arguments)."""
    out = set()
    for enc in (True, False):
        for l in plan.launches(enc):
            name = l["name"].split("::")[-1].split("<")[0]
            if "_row" in name:
                out.add(("enc" if enc else "dec", name, l["expl"], l["paired"]))
    return out


def expected_shape(cfg):
    """What a config's name promises about its row launches:
    (any explicit-tile launch, any paired launch) -- the same for both
    directions; None where the rule is the auto one's business."""
    if cfg is None:
        return True, True          # split (128 MiB waves < 256 MiB slices); pair auto = paired tables
    row2, pair, wave = cfg
    expl = row2 != 0 and wave < 256
    return expl, (pair != 0 and row2 != 0)
