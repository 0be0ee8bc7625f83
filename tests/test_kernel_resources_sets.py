"""The wakeword-set kernels (rustpotter_amd/csrc/rp_dtw_set.hip, rp_scan_sets.hip): nothing spilled and no scratch memory.  dtw_set_kernel and
dtw_set_stream_kernel run the DTW walks of the bank kernels (rp_dtw_bank.h) inside a loop over the slots of a set / over rows of slots; a
ring or band the compiler leaves rolled becomes a run-time index and the array goes to scratch memory, and scan_set_stream_kernel keeps the
slots of a set in registers behind fully unrolled loops -- exactly these counters show when either fails.  The register counts the build
gave when the kernels were written are caps.  Reads the compiler's own resource remarks (tools/kernel_regs.py compiles with the Makefile's
flags; CPU only, hipcc cross-compiles), as tests/test_kernel_resources_bank.py does."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> (source, registers of the build the kernel was written with)
KERNELS = {
    "dtw_set_kernel<5, 3>": ("rp_dtw_set.hip", 77), "dtw_set_kernel<5, 4>": ("rp_dtw_set.hip", 79),
    "dtw_set_kernel<5, 5>": ("rp_dtw_set.hip", 95), "dtw_set_kernel<5, 6>": ("rp_dtw_set.hip", 115),
    "dtw_set_kernel<13, 3>": ("rp_dtw_set.hip", 130), "dtw_set_kernel<13, 4>": ("rp_dtw_set.hip", 159),
    "dtw_set_kernel<13, 5>": ("rp_dtw_set.hip", 188), "dtw_set_kernel<13, 6>": ("rp_dtw_set.hip", 218),
    "dtw_set_kernel<16, 3>": ("rp_dtw_set.hip", 151), "dtw_set_kernel<16, 4>": ("rp_dtw_set.hip", 185),
    "dtw_set_kernel<16, 5>": ("rp_dtw_set.hip", 221), "dtw_set_kernel<16, 6>": ("rp_dtw_set.hip", 256),
    "dtw_set_stream_kernel<5, 3>": ("rp_dtw_set.hip", 92), "dtw_set_stream_kernel<5, 4>": ("rp_dtw_set.hip", 96),
    "dtw_set_stream_kernel<5, 5>": ("rp_dtw_set.hip", 110), "dtw_set_stream_kernel<5, 6>": ("rp_dtw_set.hip", 124),
    "dtw_set_stream_kernel<13, 3>": ("rp_dtw_set.hip", 154), "dtw_set_stream_kernel<13, 4>": ("rp_dtw_set.hip", 184),
    "dtw_set_stream_kernel<13, 5>": ("rp_dtw_set.hip", 216), "dtw_set_stream_kernel<13, 6>": ("rp_dtw_set.hip", 244),
    "dtw_set_stream_kernel<16, 3>": ("rp_dtw_set.hip", 174), "dtw_set_stream_kernel<16, 4>": ("rp_dtw_set.hip", 216),
    "dtw_set_stream_kernel<16, 5>": ("rp_dtw_set.hip", 250), "dtw_set_stream_kernel<16, 6>": ("rp_dtw_set.hip", 270),
    "scan_set_kernel": ("rp_scan_sets.hip", 85), "scan_set_stream_kernel": ("rp_scan_sets.hip", 143),
}


@pytest.fixture(scope="module")
def remarks():
    out = {}
    for src in sorted({s for s, _ in KERNELS.values()}):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), src, "_kernel"], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        for line in r.stdout.splitlines()[1:]:
            f = line.split(None, 7)   # vgpr agpr spill sgpr scrtch lds occ name
            if len(f) == 8:
                out[re.sub(r"^(void )?rp::", "", f[7]).strip()] = (int(f[0]) + int(f[1]), int(f[2]), int(f[4]))
    return out


def test_every_instantiation_is_listed(remarks):
    """a new (mfcc_size, band) pair of a kernel, or a new kernel in these sources, comes with its line above, or -- the two sources also hold
    the kernels of model sets and mixed sets -- with its line in the test of its own family"""
    import test_kernel_resources_mixed as mixed
    import test_kernel_resources_model_set as model_sets
    sources = {s for s, _ in KERNELS.values()}
    elsewhere = {k for t in (mixed, model_sets) for k, v in t.KERNELS.items() if v[0] in sources}
    assert not elsewhere & set(KERNELS)
    assert sorted(remarks) == sorted(set(KERNELS) | elsewhere)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_set_kernels_spill_nothing(remarks, kernel):
    assert kernel in remarks, sorted(remarks)
    regs, spill, scratch = remarks[kernel]
    print("%s: %d registers, %d spilled values, %d bytes of scratch" % (kernel, regs, spill, scratch))
    assert spill == 0, "%s: %d spilled values" % (kernel, spill)
    assert scratch == 0, "%s: %d bytes of scratch" % (kernel, scratch)
    assert regs <= KERNELS[kernel][1], "%s: %d registers, %d when it was written" % (kernel, regs, KERNELS[kernel][1])
