"""Designed planes for exact Eden decode checks (no tests here; used by
tests/test_eden_walsh_cpu.py and tests/test_gpu_eden_decode_designed.py).

For a slice of P = 2^p elements pick a centroid index k, a Walsh index j and
a rotation seed s, and give element i the bin

    k            if popcount(i & j) is even
    2^b - 1 - k  otherwise.

The centroid tables are antisymmetric (C == -C[::-1] bitwise), so the decoder
starts from C[k] * h_j, row j of the Hadamard matrix times one constant.
Every butterfly of the first transform, in any stage order, then adds or
subtracts two numbers of equal magnitude (or two zeros): each result is 0 or
twice the operand, exactly.  What is left is one spike at index j; the second
transform only adds zeros to it.  With power-of-two normalisations (DESIGN
3.4) the one rounding of the whole decode is the product with the scale:

    y[e] = fl32(scale * C[k]) * d2[j] * h_j[e] * d1[e],
    d1 = rand_diag(P, s), d2 = rand_diag(P, s + 1),

bit for bit, for every decoder that normalises by powers of two, whatever its
layouts, exchanges or stage order.  (The C oracle divides by float32(sqrt(P))
twice: it agrees bit for bit for even p only.)

Limits of the design: a run uses two bin values (k and its mirror); D2 is
probed at index j only; D1 is probed at every element.

The expectation is assembled from integer words (the bits of the one float32
product, computed in NumPy, with the sign bit flipped where the sign pattern
says so): no floating-point instruction of the device takes part in it."""
import numpy as np
import torch

from oracle import eden as O
from tests import eden_exact as X

CHUNK = 1 << 24  # elements of one size group that are built at a time


def j_set(p):
    """Walsh indices of a 2^p slice: 0, 1, P - 1, every single bit 2^t and
    three seeded random values (duplicates dropped, order kept)."""
    P = 1 << p
    rng = np.random.default_rng([4242, p])
    js = [0, 1, P - 1] + [1 << t for t in range(p)] + [int(v) for v in rng.integers(0, P, 3)]
    return list(dict.fromkeys(js))


def _parity(P, js, device):
    """[len(js), P] int32: popcount(i & j) & 1."""
    x = torch.arange(P, dtype=torch.int32, device=device)[None, :] & \
        torch.tensor(js, dtype=torch.int32, device=device)[:, None]
    for s in (16, 8, 4, 2, 1):
        x ^= x >> s
    return x.bitwise_and_(1)


def _bins_many(P, bits, ks, js, device):
    par = _parity(P, js, device)
    k = torch.tensor(ks, dtype=torch.int32, device=device)[:, None]
    return torch.where(par.bool(), (1 << bits) - 1 - k, k)


_packed_signs = X.packed_signs


def product_bits(bits, k, scale):
    """int32 words of fl32(scale * C[k]), one float32 multiply in NumPy."""
    C = O.tables(bits)[0]
    with np.errstate(all="ignore"):
        v = np.asarray(scale, np.float32) * C[np.asarray(k)]
    return v.astype(np.float32).view(np.int32)


def _expected_many(P, bits, ks, js, seeds, scales, device):
    """[S, P] int32 words of the expectation of S slices of one size."""
    S = len(ks)
    neg = _parity(P, js, device)
    d1 = np.stack([_packed_signs(P, int(s)) for s in seeds]).reshape(S, -1)
    d1 = torch.from_numpy(d1).to(device)
    sh = torch.arange(8, device=device, dtype=torch.uint8)
    plus = ((d1[:, :, None] >> sh) & 1).reshape(S, -1)[:, :P]
    neg ^= 1 - plus.to(torch.int32)
    del plus, d1
    d2 = [int(_packed_signs(P, int(s) + 1)[j >> 3] >> (j & 7)) & 1 for s, j in zip(seeds, js)]
    neg ^= 1 - torch.tensor(d2, dtype=torch.int32, device=device)[:, None]
    val = torch.from_numpy(product_bits(bits, np.asarray(ks), np.asarray(scales, np.float32))).to(device)
    return neg.mul_(-(1 << 31)) ^ val[:, None]  # the sign bit where the pattern is -1


def _pack_many(bins, bits):
    """[S, P] bins -> [S, bits, P / 8] plane bytes (to_bits order inside a slice)."""
    S, P = bins.shape
    b = bins.view(S, P // 8, 8)
    sh = torch.arange(8, device=bins.device, dtype=torch.int32)
    out = torch.empty(S, bits, P // 8, dtype=torch.uint8, device=bins.device)
    for i in range(bits):
        out[:, i] = (((b >> i) & 1) << sh).sum(2).to(torch.uint8)
    return out


def walsh_bins(P, bits, k, j, device="cpu"):
    """int32 [P]: k where popcount(i & j) is even, 2^bits - 1 - k elsewhere."""
    assert P & (P - 1) == 0 and 0 <= j < P and 0 <= k < (1 << bits)
    return _bins_many(P, bits, [k], [j], device)[0]


def walsh_expected(P, bits, k, j, seed, scale, n_valid=None, device="cpu"):
    """float32 [n_valid]: what a decoder with power-of-two normalisations
    returns, bit for bit, for walsh_bins(P, bits, k, j) under rotation seed
    `seed` and `scale`."""
    w = _expected_many(P, bits, [k], [j], [seed], [scale], device)[0]
    return w[:P if n_valid is None else n_valid].view(torch.float32)


def build_batch(plan, specs, bits, device):
    """Lay Walsh tensors into the arenas of `plan`.  specs[t] = (seed,
    [(k, j, scale) for every slice of plan.dims[t]]).  ->
      planes  uint8 [plan.planes_bytes]   (0xA5 where no tensor's planes lie)
      scales  float32 [plan.n_slices]
      seeds   int32 [tensors]
      want    int32 [plan.arena_numel]: the expected words
      valid   bool  [plan.arena_numel]: the elements a decode writes
    all on `device`.  Slices of one size are built together, CHUNK elements at
    a time."""
    assert len(specs) == len(plan.dims)
    planes = torch.full((max(plan.planes_bytes, 1),), 0xA5, dtype=torch.uint8, device=device)
    want = torch.zeros(plan.arena_numel, dtype=torch.int32, device=device)
    valid = torch.zeros(plan.arena_numel, dtype=torch.bool, device=device)
    scales = np.zeros(max(plan.n_slices, 1), np.float32)
    by_size = {}
    for t, (dims, (seed, runs)) in enumerate(zip(plan.dims, specs)):
        Ps, Ls = O.slice_plan(plan.numels[t])
        assert Ps == dims and len(runs) == len(dims), (t, dims, Ps)
        off = src = 0
        for q, (P, ln, (k, j, scale)) in enumerate(zip(Ps, Ls, runs)):
            scales[plan.first_slice[t] + q] = scale
            by_size.setdefault(P, []).append((t, off, src, ln, k, j, seed, scale))
            off += P
            src += ln
    for P, sl in by_size.items():
        step = max(1, CHUNK // P)
        for c in range(0, len(sl), step):
            part = sl[c:c + step]
            ks, js = [s[4] for s in part], [s[5] for s in part]
            packed = _pack_many(_bins_many(P, bits, ks, js, device), bits)
            words = _expected_many(P, bits, ks, js, [s[6] for s in part], [s[7] for s in part], device)
            for i, (t, off, src, ln, *_) in enumerate(part):
                po, pb = plan.planes_offsets[t], plan.planes_nbytes[t]
                planes[po:po + pb].view(bits, -1)[:, off // 8:(off + P) // 8] = packed[i]
                eo = plan.elem_offsets[t] + src
                want[eo:eo + ln] = words[i, :ln]
                valid[eo:eo + ln] = True
            del packed, words
    seeds = torch.tensor([s[0] for s in specs], dtype=torch.int32, device=device)
    return planes, torch.from_numpy(scales).to(device), seeds, want, valid


def tensor_planes(dims, bits, runs, device="cpu"):
    """The to_bits plane run of one full tensor (as oracle.eden.decompress
    reads it): slice q of `dims` holds walsh_bins(dims[q], bits, k, j) of
    runs[q] = (k, j, ...).  uint8 [bits * sum(dims) / 8]."""
    bins = torch.cat([walsh_bins(P, bits, r[0], r[1], device) for P, r in zip(dims, runs)])
    return X.expected_planes(bins, dims, bits)
