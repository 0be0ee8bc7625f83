"""Three waves per SIMD for the three-part matrix-core DTW kernel (rustpotter_amd/csrc/rp_dtw_mfma.hip): the twelve-wave builds
fit the 168 registers of a third wave with nothing spilled and no scratch memory -- a spilled value in the column loop is a store and a reload
per block and wave that reach the HBM, which is what kept the eight-slot build an opt-in.  Reads the compiler's own resource remarks
(tools/kernel_regs.py compiles with the Makefile's flags; CPU only, hipcc cross-compiles), as tests/test_kernel_resources.py does."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "rp_dtw_mfma.hip"

# kernel: (largest register count or None, spilled values, bytes of scratch or None)
CASES = {
    "dtw_mfma_kernel<5, 12, false, 8, true>": (168, 0, 0),   # the headline kernel: eight template slots, LDS-staged tiles
    "dtw_mfma_kernel<5, 12, false, 4, true>": (168, 0, 0),   # chunks of 3..4 templates
    "dtw_mfma_kernel<5, 12, true, 4, true>": (168, 0, 0),    # the same, frames from global memory
    "dtw_mfma_kernel<5, 8, false, 8, true>": (None, 0, None),  # the eight-wave build (RP_MFMA3_WAVES=8) did not pay for it
    # what a detect-only call with early abandon runs for chunks of 3..4 templates (its eight-slot form keeps the eight-wave build above)
    "dtw_mfma_abandon_kernel<5, 12, false, 4, true>": (168, 0, 0),
    "dtw_mfma_abandon_kernel<5, 12, true, 4, true>": (168, 0, 0),
}


@pytest.fixture(scope="module")
def remarks():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), SRC, "_kernel<5, "], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines()[1:]:
        f = line.split(None, 7)   # vgpr agpr spill sgpr scrtch lds occ name
        if len(f) == 8:
            out[re.sub(r"^void rp::", "", f[7]).strip()] = (int(f[0]), int(f[2]), int(f[4]))
    return out


@pytest.mark.parametrize("kernel", list(CASES))
def test_twelve_wave_builds_spill_nothing(remarks, kernel):
    assert kernel in remarks, sorted(remarks)
    max_vgpr, max_spill, max_scratch = CASES[kernel]
    vgpr, spill, scratch = remarks[kernel]
    print("%s: %d registers, %d spilled values, %d bytes of scratch" % (kernel, vgpr, spill, scratch))
    assert spill <= max_spill, "%s: %d spilled values" % (kernel, spill)
    if max_vgpr is not None:
        assert vgpr <= max_vgpr, "%s: %d registers -- no third wave per SIMD" % (kernel, vgpr)
    if max_scratch is not None:
        assert scratch <= max_scratch, "%s: %d bytes of scratch" % (kernel, scratch)
