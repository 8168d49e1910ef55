"""Designed inputs for exact Eden encode checks (no tests here; used by
tests/test_eden_exact.py, tests/test_gpu_eden_exact.py and
tests/golden/make_golden.py --only designed).

Eden rotates a slice (v = H D_{s+1} H D_s x), normalises it and buckets every
value.  Choose the bins first, set v* = alpha * C[bins] and feed the encoder
x = D_s H D_{s+1} H v*: every rotated value then sits on a centroid, well
inside its cell, so the bins are known exactly, the scale is alpha
(|v|^2 / <C[bins], v> = alpha) and decode(encode(x)) = x.  The normalised
value of bin b is C[b] / rms(C[bins]), so the construction holds only while
rms(C[bins]) keeps every used centroid inside its own cell: designed()
steers the rms and asserts the margin.

Slices whose valid length is below P (ragged: the padding has to stay zero)
cannot be designed; margin_rule() holds their bins to an fp64 rotation
instead."""
import math

import numpy as np
import torch

from oracle import eden as O

SEED = 321                     # rotation seed of every designed case
MARGIN = 2e-3                  # least distance of a normalised designed value to a boundary
NUMPY_DRAW_MAX = 1 << 23       # larger slices draw their N(0,1) on the device
WORK_MAX = 1 << 20             # elements of a slice that forcing / rebalancing may change
# the committed fixture (tests/golden/eden_designed.json): bits 1..8 at each
FIXTURE_DIMS = [[2048], [1 << 16], [1 << 20, 1 << 17]]


def case_rng(dims, bits):
    """The numpy generator that names the designed input of (dims, bits)."""
    return np.random.default_rng([SEED, int(bits)] + [int(d) for d in dims])


def default_alphas(dims):
    """0.01 for the first slice, a different scale for every further one."""
    return [0.01 * (3.7 ** k) for k in range(len(dims))]


# ------------------------------------------------------------- rotations ---
def fwht(v):
    """Orthonormal fast Walsh-Hadamard transform of a 1-D tensor of 2^p
    elements, in v's dtype on v's device: log2 P view-and-add stages, then a
    division by sqrt(P).  Returns a new tensor."""
    P = v.numel()
    assert P & (P - 1) == 0 and P > 0
    v = v.clone()
    h = 1
    while h < P:
        w = v.view(-1, 2, h)
        a = w[:, 0, :] + w[:, 1, :]
        torch.sub(w[:, 0, :], w[:, 1, :], out=w[:, 1, :])
        w[:, 0, :] = a
        del a
        h *= 2
    return v.div_(math.sqrt(P))


_packed = {}
_packed_bytes = 0
PACKED_CACHE_BYTES = 1 << 27


def packed_signs(P, seed):
    """oracle.eden.rand_signs(P, seed), kept (the oracle hashes on one thread:
    0.5 s at 2^26) while the kept arrays stay below PACKED_CACHE_BYTES."""
    global _packed_bytes
    key = (int(P), int(seed))
    if key not in _packed:
        if _packed_bytes + (P + 7) // 8 > PACKED_CACHE_BYTES:
            _packed.clear()
            _packed_bytes = 0
        _packed[key] = O.rand_signs(P, seed)
        _packed[key].setflags(write=False)
        _packed_bytes += _packed[key].nbytes
    return _packed[key]


def signs(P, seed, dtype, device):
    """rand_diag(P, seed) as a +-1 tensor, from oracle.eden.rand_signs."""
    packed = torch.tensor(packed_signs(P, seed), device=device)  # a copy: the kept array is read-only
    bit = (packed[:, None] >> torch.arange(8, device=device, dtype=torch.uint8)[None, :]) & 1
    return bit.reshape(-1)[:P].to(dtype).mul_(2).sub_(1)


def rotate(x_padded, seed):
    """H D_{seed+1} H D_seed x: what the encoder buckets (before normalising)."""
    v = fwht(x_padded * signs(x_padded.numel(), seed, x_padded.dtype, x_padded.device))
    return fwht(v.mul_(signs(v.numel(), seed + 1, v.dtype, v.device)))


def unrotate(v, seed):
    """D_seed H D_{seed+1} H v: the inverse of rotate()."""
    x = fwht(v).mul_(signs(v.numel(), seed + 1, v.dtype, v.device))
    return fwht(x).mul_(signs(v.numel(), seed, v.dtype, v.device))


# -------------------------------------------------------- designed inputs ---
def _tables64(bits):
    C, B = O.tables(bits)
    return C.astype(np.float64), B.astype(np.float64)


def cell_margin(hist, P, bits):
    """fp64: min over the used bin values b of the distance of
    C[b] / rms(C[bins]) to the nearer boundary of b's own cell (negative when
    a value leaves its cell).  hist: occurrences of every bin value."""
    C, B = _tables64(bits)
    r = math.sqrt(float(np.dot(hist.astype(np.float64), C * C)) / P)
    return _margin_at(r, hist > 0, C, B)


def _margin_at(r, used, C, B):
    z = C / r
    lo = np.concatenate(([-np.inf], B))
    hi = np.concatenate((B, [np.inf]))
    return float(np.min(np.minimum(z - lo, hi - z)[used]))


def _best_rms(used, C, B):
    """The rms(C[bins]) in [0.97, 1.03] that leaves the used values the most room."""
    grid = np.linspace(0.97, 1.03, 1201)
    return float(grid[int(np.argmax([_margin_at(r, used, C, B) for r in grid]))])


def _rebalance(sub, free, hist, P, bits, rng, distinct):
    """Move rms(C[bins]) to the value that centres the used centroids in their
    cells, changing only free elements of `sub` (and `hist` with them): a
    coarse step that sends random elements to a centre bin (too much energy,
    the usual case after forcing the outer bins) or to the bins at
    |C| ~ sqrt(2) (too little), then single elements chosen to close the rest.
    distinct: prefer bin values that no element uses yet (small slices)."""
    C, B = _tables64(bits)
    C2 = C * C
    nv = 1 << bits
    if nv == 2:
        return  # |C| is the same for both values: the rms is what it is
    S = float(np.dot(hist.astype(np.float64), C2))
    T = P * _best_rms(hist > 0, C, B) ** 2
    idx = np.flatnonzero(free)

    def move(i, b):
        nonlocal S
        S += C2[b] - C2[sub[i]]
        hist[sub[i]] -= 1
        hist[b] += 1
        sub[i] = b

    if idx.size >= 1024 and abs(S - T) > 2.0:
        d = S - T
        perm = rng.permutation(idx)[:int(4 * abs(d)) + 64]
        if d > 0:
            tgt = np.where(rng.random(perm.size) < 0.5, nv // 2 - 1, nv // 2)
        else:
            k = int(np.argmin(np.abs(C - math.sqrt(2.0))))
            tgt = np.where(rng.random(perm.size) < 0.5, k, nv - 1 - k)
        gain = (C2[sub[perm]] - C2[tgt]) * (1 if d > 0 else -1)
        ok = gain > 0
        perm, tgt, gain = perm[ok], tgt[ok], gain[ok]
        n = int(np.searchsorted(np.cumsum(gain), abs(d)))
        for i, b in zip(perm[:n], tgt[:n]):
            move(i, b)
    want = 0.9 * _margin_at(math.sqrt(T / P), hist > 0, C, B)
    for _ in range(2000):
        if _margin_at(math.sqrt(S / P), hist > 0, C, B) >= max(want, 2 * MARGIN) or idx.size == 0:
            break
        i = int(idx[rng.integers(idx.size)])
        need = T - (S - C2[sub[i]])
        b = int(np.argmin(np.abs(C2 - need)))
        if distinct and np.any(hist == 0):  # an unused value, where it serves about as well
            un = np.flatnonzero(hist == 0)
            u = int(un[np.argmin(np.abs(C2[un] - need))])
            if abs(C2[u] - need) <= 0.25 * abs(S - T):
                b = u
        if abs(C2[b] - need) < abs(S - T):
            move(i, b)


def _design_slice(P, bits, rng, device, force_each, rebalance):
    nv = 1 << bits
    Bt = torch.from_numpy(O.tables(bits)[1]).to(device)
    if P <= NUMPY_DRAW_MAX:
        z = torch.from_numpy(rng.standard_normal(P, dtype=np.float32)).to(device)
    else:
        g = torch.Generator(device=device).manual_seed(int(rng.integers(1 << 62)))
        z = torch.empty(P, dtype=torch.float32, device=device).normal_(generator=g)
    bins = torch.bucketize(z, Bt, out_int32=True)
    del z
    hist = torch.bincount(bins, minlength=nv).cpu().numpy().astype(np.int64)
    # the elements that forcing and rebalancing may change: a strided subset
    m = min(P, WORK_MAX)
    stride = P // m
    widx = torch.arange(m, device=device) * stride + int(rng.integers(stride))
    sub = bins[widx].cpu().numpy().astype(np.int64)
    hist -= np.bincount(sub, minlength=nv)
    free = np.ones(m, bool)
    if P >= 4 * nv:        # every bin value, both outermost ones included
        k = force_each * nv
        seg = m // k
        pos = seg * np.arange(k) + rng.integers(0, seg, k)
        sub[pos] = rng.permutation(np.tile(np.arange(nv), force_each))
        free[pos] = False
    else:                  # as many distinct values as fit: duplicates move to the nearest unused value
        cnt = np.bincount(sub, minlength=nv)
        for i in rng.permutation(m):
            if cnt[sub[i]] > 1 and np.any(cnt == 0):
                un = np.flatnonzero(cnt == 0)
                b = int(un[np.argmin(np.abs(un - sub[i]))])
                cnt[sub[i]] -= 1
                cnt[b] += 1
                sub[i] = b
    hist += np.bincount(sub, minlength=nv)
    if rebalance:
        _rebalance(sub, free, hist, P, bits, rng, distinct=P < 4 * nv)
    bins[widx] = torch.from_numpy(sub).to(device=device, dtype=torch.int32)
    got = torch.bincount(bins, minlength=nv).cpu().numpy()
    assert np.array_equal(got, hist)
    margin = cell_margin(got, P, bits)
    assert margin >= MARGIN, f"designed slice P={P} bits={bits}: margin {margin:.3e} < {MARGIN}"
    if P >= 4 * nv:
        assert np.all(got > 0)
    return bins, margin


def designed(dims, bits, seed=SEED, alphas=None, rng=None, device="cpu", force_each=1, rebalance=True):
    """-> (x fp32 [sum(dims)], bins int32 [sum(dims)], alphas): slice k of x is
    D_s H D_{s+1} H (alphas[k] * C[bins of slice k]) computed in fp64, so that
    an Eden encoder with rotation seed `seed` must return exactly `bins` and
    the scales `alphas`.  Every slice is full (len == P = dims[k]), and
    sum(dims) must slice into dims.  In a slice with P >= 4 * 2^bits every bin
    value occurs (force_each times at least); a smaller slice gets as many
    distinct values as the draw and the margin leave room for.  The rest is
    N(0,1) bucketised, drawn from `rng` (default case_rng(dims, bits); slices
    above NUMPY_DRAW_MAX draw on the device from a torch generator that rng
    seeds).  Asserts, in fp64, that every normalised designed value
    C[bin] / rms(C[bins]) lies at least MARGIN inside its own cell.
    force_each / rebalance=False exist to show that assertion firing."""
    dims = [int(d) for d in dims]
    assert O.slice_plan(sum(dims))[0] == dims, (dims, O.slice_plan(sum(dims)))
    alphas = default_alphas(dims) if alphas is None else [float(a) for a in alphas]
    assert len(alphas) == len(dims)
    rng = case_rng(dims, bits) if rng is None else rng
    C = torch.from_numpy(O.tables(bits)[0].astype(np.float64)).to(device)
    xs, bs = [], []
    for P, alpha in zip(dims, alphas):
        bins, _ = _design_slice(P, bits, rng, device, force_each, rebalance)
        v = C[bins.long()].mul_(alpha)
        xs.append(unrotate(v, seed).float())
        bs.append(bins)
        del v
    return (torch.cat(xs) if len(xs) > 1 else xs[0]), (torch.cat(bs) if len(bs) > 1 else bs[0]), alphas


def expected_planes(bins, dims, bits):
    """The reference's to_bits layout over the whole tensor (as
    oracle.eden.bins_of reads it): plane i at byte offset i * L, L = sum(dims)
    / 8; bit t of byte j of plane i = bit i of bins[8 j + t].  uint8 tensor on
    bins' device."""
    Ptot = int(sum(dims))
    assert bins.numel() == Ptot and Ptot % 8 == 0
    b = bins.view(Ptot // 8, 8)
    sh = torch.arange(8, device=bins.device, dtype=b.dtype)[None, :]
    out = torch.empty(bits, Ptot // 8, dtype=torch.uint8, device=bins.device)
    for i in range(bits):
        out[i] = (((b >> i) & 1) << sh).sum(1).to(torch.uint8)
    return out.reshape(-1)


def bins_from_planes(planes, Ptot, bits):
    """expected_planes' inverse on the device: int32 bins of a to_bits plane run."""
    p = planes.view(bits, Ptot // 8)
    sh = torch.arange(8, device=planes.device, dtype=torch.uint8)[None, :]
    out = torch.zeros(Ptot, dtype=torch.int32, device=planes.device)
    for i in range(bits):
        out += ((p[i][:, None] >> sh) & 1).reshape(-1).to(torch.int32) << i
    return out


# ------------------------------------------------------------ ragged slices ---
def rotated64(x, n, dims, seed):
    """Per slice of the reference's slicing of n: the zero-padded slice of x
    (fp32, n elements) rotated in fp64 on x's device."""
    Ps, Ls = O.slice_plan(n)
    assert Ps == [int(d) for d in dims]
    out, src = [], 0
    for P, ln in zip(Ps, Ls):
        pad = torch.zeros(P, dtype=torch.float64, device=x.device)
        pad[:ln] = x[src:src + ln].double()
        out.append(rotate(pad, seed))
        src += ln
    return out


def _oracle_rotated32(x_slice, P, seed):
    """The oracle's own fp32 rotation of a zero-padded slice (numpy, CPU)."""
    w = np.zeros(P, np.float32)
    w[:x_slice.size] = x_slice
    for i in range(2):
        w = O.fwht(w * O.rand_diag(P, seed + i))
    return w


def margin_rule(x, n, dims, bits, seed, got_bins, v64=None):
    """Hold an encoder's bins on slices that cannot be designed to an fp64
    rotation.  z = v64 * sqrt(P) / |v64| is bucketed in fp64; an element farther
    than tau from every boundary must have exactly the fp64 bin; a nearer one
    may have that bin or the one on the other side of that same boundary,
    nothing else.  tau = 4 x the oracle's own worst |v32 - v64| * sqrt(P) / |v|
    on this input (its fp32 rotation against the fp64 one), the factor for an
    encoder that butterflies in another order.  Asserts the rule; returns the
    share of elements inside tau."""
    v64 = rotated64(x, n, dims, seed) if v64 is None else v64
    _, B = _tables64(bits)
    Bt = torch.from_numpy(B).to(x.device)
    lo = torch.cat((torch.tensor([-math.inf], dtype=torch.float64, device=x.device), Bt))
    hi = torch.cat((Bt, torch.tensor([math.inf], dtype=torch.float64, device=x.device)))
    Ps, Ls = O.slice_plan(n)
    inside = 0
    off = src = 0
    for P, ln, v in zip(Ps, Ls, v64):
        nrm = float(torch.linalg.vector_norm(v))
        v32 = _oracle_rotated32(x[src:src + ln].cpu().numpy(), P, seed)
        dev = float((torch.from_numpy(v32).to(x.device).double() - v).abs().max()) * math.sqrt(P) / nrm
        tau = 4.0 * dev
        z = v * (math.sqrt(P) / nrm)
        b64 = torch.bucketize(z, Bt)
        dlo, dhi = z - lo[b64], hi[b64] - z
        dist = torch.minimum(dlo, dhi)
        other = torch.where(dlo < dhi, b64 - 1, b64 + 1)
        got = got_bins[off:off + P].long()
        near = dist <= tau
        bad_far = int(((got != b64) & ~near).sum())
        bad_near = int(((got != b64) & (got != other) & near).sum())
        assert bad_far == 0 and bad_near == 0, \
            f"slice P={P}: {bad_far} elements farther than tau={tau:.2e} from a boundary off their fp64 bin, " \
            f"{bad_near} nearer ones in neither neighbouring bin"
        inside += int(near.sum())
        off += P
        src += ln
    return inside / float(sum(Ps))
