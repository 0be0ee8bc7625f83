"""stream_targets_kernel (rustpotter_amd/csrc/rp_gain_targets.hip), the preparation kernel in front of the per-stream gain kernels: nothing
spilled and no scratch memory -- a lane folds at most two rows of eight indices into a length and a level.  Reads the compiler's own resource remarks
(tools/kernel_regs.py compiles with the Makefile's flags; CPU only, hipcc cross-compiles), as tests/test_kernel_resources_bank_put.py does."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "rp_gain_targets.hip"
KERNELS = ["stream_targets_kernel"]


@pytest.fixture(scope="module")
def remarks():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), SRC, "_kernel"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines()[1:]:
        f = line.split(None, 7)   # vgpr agpr spill sgpr scrtch lds occ name
        if len(f) == 8:
            out[re.sub(r"\(.*$", "", re.sub(r"^(void )?rp::", "", f[7])).strip()] = (int(f[0]), int(f[2]), int(f[4]))
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_gain_targets_kernel_spills_nothing(remarks, kernel):
    assert kernel in remarks, sorted(remarks)
    vgpr, spill, scratch = remarks[kernel]
    print("%s: %d registers, %d spilled values, %d bytes of scratch" % (kernel, vgpr, spill, scratch))
    assert spill == 0, "%s: %d spilled values" % (kernel, spill)
    assert scratch == 0, "%s: %d bytes of scratch" % (kernel, scratch)
