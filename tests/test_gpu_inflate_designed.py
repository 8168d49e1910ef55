"""k_inflate_members on designed deflate streams (tests/deflate_cases.py), with
zlib as the reference: every block type and header count, every length and
distance code at both ends of its extra bits, the copy paths either side of
the 64-lane width and of the 1 KiB ring, code lengths that take the canonical
walk, stored blocks after every bit offset, the CRC tree at every alignment;
and, for each check in the kernel that refuses a member, a stream that only
that check can refuse, next to an intact twin that must decode on the same
buffers.  The same tables run under the opt-in decoder variants in a child
process each."""
import gzip
import os
import subprocess
import sys
import zlib

import pytest

from tests import deflate_cases as dc
from tests import deflate_device as dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", dc.valid_cases(), ids=lambda c: c.name)
def test_valid_stream_equals_zlib(case):
    want = b"".join(zlib.decompress(m.body, -15) for m in case.members)
    assert want == case.data == gzip.decompress(case.stream)
    assert dev.inflate_members(case.stream) == want          # the kernel, called as the fallback calls it
    assert dev.gunzip_device(case.stream, len(want)) == want


@pytest.mark.parametrize("case", dc.invalid_cases(), ids=lambda c: c.name)
def test_invalid_stream_is_refused(case):
    """zlib raises on these bytes, so the device must: CodecError from both
    entry points, then the intact twin decodes on the same buffers."""
    with pytest.raises((zlib.error, EOFError, OSError)):
        gzip.decompress(case.stream)
    assert dev.invalid_verdict(case) == "refused"


@pytest.mark.parametrize("variant", ["OFL_GZ_INFLATE=window", "OFL_GZ_PAIR=1"])
def test_opt_in_variant_gives_the_same_verdicts(variant):
    """The LDS-window decoder (16 and 64 KiB windows) and the pair table are
    chosen once per process by the environment: the same two tables in a
    fresh child process under each."""
    key, val = variant.split("=")
    env = dict(os.environ, **{key: val})
    env.pop("OFL_GZ_PAIR" if key == "OFL_GZ_INFLATE" else "OFL_GZ_INFLATE", None)
    r = subprocess.run([sys.executable, "-m", "tests.deflate_device"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if "\t" in ln]
    got = dict(ln.split("\t", 1) for ln in lines)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("done"), r.stdout[-2000:] + r.stderr[-2000:]
    want = {f"valid {c.name}": "ok" for c in dc.valid_cases()}
    want.update({f"invalid {c.name}": "refused" for c in dc.invalid_cases()})
    assert {k: v for k, v in got.items() if want.get(k) != v} == {} and got.keys() == want.keys()
