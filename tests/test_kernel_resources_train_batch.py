"""The batched trainer's kernel (rustpotter_amd/csrc/rp_train_batch.hip): nothing spilled and no scratch memory.  The kernel walks a
model's layers through the job table in global memory; a job copied into registers and indexed by the layer would go to scratch, and a
spilled value in the dot-product loops would be a store and a reload per step of every epoch.  Reads the compiler's own resource remarks
(tools/kernel_regs.py compiles with the Makefile's flags; CPU only, hipcc cross-compiles), as tests/test_kernel_resources_average.py
does."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "rp_train_batch.hip"


@pytest.fixture(scope="module")
def remarks():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), SRC, "_kernel"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines()[1:]:
        f = line.split(None, 7)   # vgpr agpr spill sgpr scrtch lds occ name
        if len(f) == 8:
            out[re.sub(r"^(void )?rp::", "", f[7]).strip()] = (int(f[0]), int(f[2]), int(f[4]))
    return out


def test_train_batch_kernel_spills_nothing(remarks):
    assert "train_batch_kernel" in remarks, sorted(remarks)
    vgpr, spill, scratch = remarks["train_batch_kernel"]
    print("train_batch_kernel: %d registers, %d spilled values, %d bytes of scratch" % (vgpr, spill, scratch))
    assert vgpr <= 128, "a workgroup of 1024 threads leaves a thread 128 registers"
    assert spill == 0, "%d spilled values" % spill
    assert scratch == 0, "%d bytes of scratch" % scratch
