"""The kernels of a live-stream batch over a wakeword bank (dtw_bank_stream_kernel in rustpotter_amd/csrc/rp_dtw_bank.hip,
scan_bank_stream_kernel in rp_scan.hip): nothing spilled and no scratch memory.  dtw_bank_stream_kernel calls bank_dtw with per-lane template
lengths and rows; the band's ring of unit-length frames and the running costs must still sit in registers behind compile-time indices -- a
ring or band the compiler leaves rolled becomes a run-time index, the array goes to scratch memory and exactly these counters show it.  The
register counts (vector + accumulation registers) the build gave when the kernels were written are caps: a build that needs more has lost
occupancy, and at (16, 6), which already takes every vector register, would start to spill.  Reads the compiler's own resource remarks
(tools/kernel_regs.py compiles with the Makefile's flags; CPU only, hipcc cross-compiles), as tests/test_kernel_resources_bank.py does."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> (source, registers of the build the kernel was written with)
KERNELS = {
    "dtw_bank_stream_kernel<5, 3>": ("rp_dtw_bank.hip", 92), "dtw_bank_stream_kernel<5, 4>": ("rp_dtw_bank.hip", 96),
    "dtw_bank_stream_kernel<5, 5>": ("rp_dtw_bank.hip", 110), "dtw_bank_stream_kernel<5, 6>": ("rp_dtw_bank.hip", 124),
    "dtw_bank_stream_kernel<13, 3>": ("rp_dtw_bank.hip", 154), "dtw_bank_stream_kernel<13, 4>": ("rp_dtw_bank.hip", 184),
    "dtw_bank_stream_kernel<13, 5>": ("rp_dtw_bank.hip", 216), "dtw_bank_stream_kernel<13, 6>": ("rp_dtw_bank.hip", 244),
    "dtw_bank_stream_kernel<16, 3>": ("rp_dtw_bank.hip", 174), "dtw_bank_stream_kernel<16, 4>": ("rp_dtw_bank.hip", 216),
    "dtw_bank_stream_kernel<16, 5>": ("rp_dtw_bank.hip", 250), "dtw_bank_stream_kernel<16, 6>": ("rp_dtw_bank.hip", 270),
    "scan_bank_stream_kernel": ("rp_scan.hip", 96),
}


@pytest.fixture(scope="module")
def remarks():
    out = {}
    for src in sorted({s for s, _ in KERNELS.values()}):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), src, "_bank_stream_kernel"], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        for line in r.stdout.splitlines()[1:]:
            f = line.split(None, 7)   # vgpr agpr spill sgpr scrtch lds occ name
            if len(f) == 8:
                out[re.sub(r"^(void )?rp::", "", f[7]).strip()] = (int(f[0]) + int(f[1]), int(f[2]), int(f[4]))
    return out


def test_every_instantiation_is_listed(remarks):
    """a new (mfcc_size, band) pair of the kernel comes with its line above"""
    assert sorted(remarks) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_stream_bank_kernels_spill_nothing(remarks, kernel):
    assert kernel in remarks, sorted(remarks)
    regs, spill, scratch = remarks[kernel]
    print("%s: %d registers, %d spilled values, %d bytes of scratch" % (kernel, regs, spill, scratch))
    assert spill == 0, "%s: %d spilled values" % (kernel, spill)
    assert scratch == 0, "%s: %d bytes of scratch" % (kernel, scratch)
    assert regs <= KERNELS[kernel][1], "%s: %d registers, %d when it was written" % (kernel, regs, KERNELS[kernel][1])
