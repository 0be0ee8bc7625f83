"""The register DTW kernels of rp_dtw.hip sit on the register cliff: several band 5 / 6 builds of dtw_band_kernel and the mfcc_size 16 builds of
dtw_band_wide_kernel use all 256 registers, <5, 6, 8> spills a handful of values, and most run one or two waves per SIMD.  The per-lane walk
they share (csrc/rp_dtw_lane.h) is expanded into each of them, so a change to a shared piece moves every build at once.  This test reads the
compiler's resource remarks (tools/kernel_regs.py, the Makefile's flags; CPU only) and holds the cliff builds to the numbers they had when the
walk was folded into one header.  (dtw_bank_kernel and dtw_set_kernel, the other users of that header, are bound at every (mfcc_size, band) by
test_kernel_resources_bank.py and test_kernel_resources_sets.py.)"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "rp_dtw.hip"

# (kernel, largest number of spilled registers accepted, largest register count)
CASES = [
    ("dtw_band_kernel<5, 5, 8, false>", 0, 256),        # the staged strict_f32 kernel of eight templates at the default band
    ("dtw_band_kernel<5, 6, 8, false>", 7, 256),
    ("dtw_band_kernel<5, 6, 8, true>", 6, 256),
    ("dtw_band_wide_kernel<16, 6, 2, true>", 0, 256),
    ("dtw_band_wide_kernel<16, 5, 2, false>", 0, 215),
    ("dtw_band2_kernel<5, 5, false>", 0, 166),
]


@pytest.fixture(scope="module")
def remarks():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), SRC], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines()[1:]:
        f = line.split(None, 7)
        if len(f) == 8:
            out[re.sub(r"^void rp::", "", f[7]).strip()] = (int(f[0]), int(f[2]))
    return out


@pytest.mark.parametrize("kernel,max_spill,max_vgpr", CASES)
def test_cliff_builds_keep_their_registers(remarks, kernel, max_spill, max_vgpr):
    assert kernel in remarks, sorted(remarks)
    vgpr, spill = remarks[kernel]
    assert spill <= max_spill and vgpr <= max_vgpr, "%s: %d registers, %d spilled (bounds %d, %d)" % (kernel, vgpr, spill, max_vgpr, max_spill)
