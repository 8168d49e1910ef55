"""The gzip codec sets up a device once, from whichever entry point runs first
(the CRC tables in constant memory and the two kernels' dynamic-LDS sizes):
each of three fresh processes makes a different library call its first one
and must get the right bytes.  (`python -m tests.test_gpu_gzip_first_call
WHICH` is the child.)"""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CHILDREN = {"encode": {}, "tlz_decode": {}, "window_inflate": {"OFL_GZ_INFLATE": "window"}}


def _window_case():
    """A valid stream whose largest member gives 16 KiB < bytes <= 64 KiB: the 64 KiB window kernel."""
    from tests import deflate_cases as dc
    for c in dc.valid_cases():
        if 16384 < max(len(m.data) for m in c.members) <= 65536:
            return c
    raise AssertionError("no valid case of that size")


def child(which):
    import torch
    assert torch.cuda.is_available()
    if which == "encode":
        from openfl_amd import lossy
        x = np.random.default_rng(5).integers(0, 6, 2049).astype(np.float32)      # one member, two segments
        z = lossy.gzip_ranks(torch.from_numpy(x).to("cuda:0"))
        assert gzip.decompress(z) == x.tobytes()
    elif which == "tlz_decode":
        from tests import deflate_cases as dc
        from tests.deflate_device import tlz_decode
        m = dc.seven_segments()
        assert tlz_decode(m.z) == ("accepted", m.data)
    else:
        from tests.deflate_device import inflate_members
        assert os.environ.get("OFL_GZ_INFLATE") == "window"
        c = _window_case()
        assert inflate_members(c.stream) == c.data
    print(f"first call {which}: ok", flush=True)


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(CHILDREN))
def test_first_library_call(which):
    env = dict(os.environ, **CHILDREN[which])
    if which != "window_inflate":
        env.pop("OFL_GZ_INFLATE", None)
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_gzip_first_call", which], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"first call {which}: ok" in r.stdout


if __name__ == "__main__":
    child(sys.argv[1])
