"""Drivers of the device inflate kernels for the designed-stream tests: the
generic member inflate called as lossy.gunzip_device's fallback calls it
(ofl_gzip_member_index + ofl_inflate_members), the TLZ decoder alone
(ofl_inflate_tlz_async + ofl_inflate_tlz_check, whose verdict the production
path hides behind its fallback), and the verdict table a child process prints
when the inflate tests run under an opt-in decoder variant
(`python -m tests.deflate_device`, one line per case)."""
import ctypes
import sys

import numpy as np

MARK = 0xA5
SPARE = 64
DEV = "cuda:0"


def _index(L, src):
    from openfl_amd import _lib
    cap = src.size // 26 + 1
    idx = np.empty((cap, 4), np.int64)
    nm, tot, mx, tl = ctypes.c_int64(), ctypes.c_size_t(), ctypes.c_uint32(), ctypes.c_int()
    _lib.check_gzip(L.ofl_gzip_member_index(src.ctypes.data, src.size, idx.ctypes.data, cap, ctypes.byref(nm),
                                            ctypes.byref(tot), ctypes.byref(mx), ctypes.byref(tl)))
    return idx[:nm.value].copy(), tot.value, mx.value, tl.value


def _device_stream(src):
    """The stream in a 16-byte aligned device buffer followed by 128 zero bytes."""
    import torch
    d_in = torch.zeros(src.size + 128, dtype=torch.uint8, device=DEV)
    d_in[:src.size] = torch.from_numpy(src.copy())
    assert d_in.data_ptr() % 16 == 0
    return d_in


def inflate_members(z, out=None):
    """ofl_inflate_members on stream z -> the output bytes.  out: a marker-filled
    device buffer to decode into (allocated to fit when None); the SPARE bytes
    after the output must keep the marker.  Raises CodecError as the kernel's
    status says."""
    import torch
    from openfl_amd import _lib
    L = _lib.lib()
    src = np.frombuffer(z, np.uint8)
    idx, total, mx, _ = _index(L, src)
    d_in = _device_stream(src)
    d_idx = torch.from_numpy(idx).to(DEV)
    if out is None:
        out = torch.full((total + SPARE,), MARK, dtype=torch.uint8, device=DEV)
    assert out.numel() >= total + SPARE
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    rc = L.ofl_inflate_members(d_in.data_ptr(), d_idx.data_ptr(), idx.shape[0], mx, out.data_ptr(), total,
                               ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[total:total + SPARE] == MARK).all(), "bytes written past the output"
    _lib.check_gzip(rc)
    return host[:total].tobytes()


def tlz_decode(z, lut=None):
    """The TLZ decoder alone on stream z: ('accepted', bytes) or ('refused',
    None).  No fallback: k_tlz_ops and k_tlz_resolve, then their verdict."""
    import torch
    from openfl_amd import _lib
    L = _lib.lib()
    src = np.frombuffer(z, np.uint8)
    idx, total, _, all_tlz = _index(L, src)
    assert all_tlz == 1, "the index does not take every member for TLZ"
    nm = idx.shape[0]
    d_in = _device_stream(src)
    d_idx = torch.from_numpy(idx).to(DEV)
    out = torch.full((total + SPARE,), MARK, dtype=torch.uint8, device=DEV)
    wsb = int(L.ofl_inflate_tlz_workspace_bytes(nm))
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check_gzip(L.ofl_inflate_tlz_async(d_in.data_ptr(), d_idx.data_ptr(), 0, nm, out.data_ptr(), total,
                                            ws.data_ptr(), wsb, st))
    rc = L.ofl_inflate_tlz_check(nm, ws.data_ptr(), wsb, st)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[total:total + SPARE] == MARK).all(), "bytes written past the output"
    if rc == _lib.OFL_EFORMAT:
        return "refused", None
    _lib.check_gzip(rc)
    return "accepted", host[:total].tobytes()


def gunzip_device(z, nbytes):
    import torch
    from openfl_amd import lossy
    out = torch.full((nbytes + SPARE,), MARK, dtype=torch.uint8, device=DEV)
    got = lossy.gunzip_device(z, out)
    assert int(out[nbytes:].eq(MARK).all()), "bytes written past the output"
    return got.cpu().numpy().tobytes()


def valid_verdict(case):
    """'ok', or what went wrong, for a valid case on both device paths."""
    from openfl_amd import _lib
    try:
        if inflate_members(case.stream) != case.data:
            return "wrong bytes (ofl_inflate_members)"
        if gunzip_device(case.stream, len(case.data)) != case.data:
            return "wrong bytes (gunzip_device)"
    except (_lib.CodecError, AssertionError) as e:
        return f"error: {e}"
    return "ok"


def invalid_verdict(case):
    """'refused' when the device raises CodecError on the bad stream (with the
    expected text) and then decodes the intact twin on the same buffers."""
    import re
    import torch
    from openfl_amd import _lib
    out = torch.full((len(case.twin_data) + 4096 + SPARE,), MARK, dtype=torch.uint8, device=DEV)
    for fn in (lambda s: inflate_members(s, out), lambda s: gunzip_device(s, len(case.twin_data) + 4096)):
        try:
            fn(case.stream)
            return "accepted"
        except _lib.CodecError as e:
            if case.match and not re.search(case.match, str(e)):
                return f"refused, but with: {e}"
        except AssertionError as e:
            return f"error: {e}"
        out.fill_(MARK)
        try:
            if fn(case.twin) != case.twin_data:
                return "twin: wrong bytes"
        except (_lib.CodecError, AssertionError) as e:
            return f"twin: {e}"
        out.fill_(MARK)
    return "refused"


def main():
    from tests import deflate_cases as dc
    for case in dc.valid_cases():
        print(f"valid {case.name}\t{valid_verdict(case)}", flush=True)
    for case in dc.invalid_cases():
        print(f"invalid {case.name}\t{invalid_verdict(case)}", flush=True)
    print("done", flush=True)


if __name__ == "__main__":
    sys.exit(main())
