"""scan_kernel and scan_stream_kernel (rustpotter_amd/csrc/rp_scan.hip): nothing spilled, no scratch memory, three workgroups' worth of
occupancy.  All four scan kernels run one state machine (scan_frames) through closures; a closure that captures the wakewords by value, or a
shared piece the compiler does not inline, shows here as scratch memory or spills.  The occupancy remark of 3 is set by LDS, not by registers
(a one-wave workgroup holds the 12.8 KB of VAD windows of its 64 streams), so no register cap is asserted for these two; the counts are
printed.  The two bank forms have their caps in tests/test_kernel_resources_bank.py and tests/test_kernel_resources_stream_bank.py.  Reads
the compiler's own resource remarks (tools/kernel_regs.py compiles with the Makefile's flags; CPU only, hipcc cross-compiles)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["scan_kernel", "scan_stream_kernel"]


@pytest.fixture(scope="module")
def remarks():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "rp_scan.hip", "scan_"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines()[1:]:
        f = line.split(None, 7)   # vgpr agpr spill sgpr scrtch lds occ name
        if len(f) == 8:
            out[re.sub(r"^(void )?rp::", "", f[7]).strip()] = (int(f[0]) + int(f[1]), int(f[2]), int(f[4]), int(f[6]))
    return out


def test_the_scan_kernels_are_the_four(remarks):
    """a fifth kernel on the shared state machine comes with its resource test"""
    assert sorted(remarks) == ["scan_bank_kernel", "scan_bank_stream_kernel", "scan_kernel", "scan_stream_kernel"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_scan_kernels_spill_nothing(remarks, kernel):
    assert kernel in remarks, sorted(remarks)
    regs, spill, scratch, occupancy = remarks[kernel]
    print("%s: %d registers, %d spilled values, %d bytes of scratch, occupancy %d" % (kernel, regs, spill, scratch, occupancy))
    assert spill == 0, "%s: %d spilled values" % (kernel, spill)
    assert scratch == 0, "%s: %d bytes of scratch" % (kernel, scratch)
    assert occupancy == 3, "%s: occupancy %d" % (kernel, occupancy)
