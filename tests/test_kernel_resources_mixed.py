"""The mixed-set kernels (rustpotter_amd/csrc/rp_gain_targets.hip, rp_scan_sets.hip, rp_dtw_set.hip, rp_mlp_mixed.hip): nothing spilled and
no scratch memory.  stream_targets_kernel folds two rows of up to eight indices per lane; the scan kernels run the detection state machine
(scan_frames) over both kinds, scan_mixed_set_stream_kernel with the slots of both rows in registers behind fully unrolled loops;
dtw_mixed_stream_kernel runs the DTW walks of the bank kernels (rp_dtw_bank.h) per lane and the forward fronts share the bodies of the
model-set kernels -- a ring, band or slot array the compiler leaves rolled becomes a run-time index and goes to scratch memory, which shows in
exactly these counters.  The register counts the build gave when the kernels were written
are caps.  Reads the compiler's own resource remarks (tools/kernel_regs.py compiles with the Makefile's flags; CPU only, hipcc
cross-compiles), as tests/test_kernel_resources_sets.py does."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> (source, registers of the build the kernel was written with)
KERNELS = {
    "stream_targets_kernel": ("rp_gain_targets.hip", 14),
    "scan_mixed_set_kernel": ("rp_scan_sets.hip", 97), "scan_mixed_set_stream_kernel": ("rp_scan_sets.hip", 199),
    "dtw_mixed_stream_kernel<16, 3>": ("rp_dtw_set.hip", 174), "dtw_mixed_stream_kernel<16, 4>": ("rp_dtw_set.hip", 216),
    "dtw_mixed_stream_kernel<16, 5>": ("rp_dtw_set.hip", 250), "dtw_mixed_stream_kernel<16, 6>": ("rp_dtw_set.hip", 270),
    "window_means_mixed_stream_kernel": ("rp_mlp_mixed.hip", 40),
    "mlp_mixed_stream_kernel<1>": ("rp_mlp_mixed.hip", 132), "mlp_mixed_stream_kernel<2>": ("rp_mlp_mixed.hip", 173),
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


def test_every_kernel_is_listed(remarks):
    """a new kernel in these sources comes with its line above, or -- rp_dtw_set.hip and rp_scan_sets.hip also hold the kernels of wakeword
    sets and model sets -- with its line in the test of its own family"""
    import test_kernel_resources_model_set as model_sets
    import test_kernel_resources_sets as sets
    sources = {s for s, _ in KERNELS.values()}
    elsewhere = {k for t in (sets, model_sets) for k, v in t.KERNELS.items() if v[0] in sources}
    assert not elsewhere & set(KERNELS)
    assert sorted(remarks) == sorted(set(KERNELS) | elsewhere)


def test_the_sources_are_part_of_the_build():
    mk = open(os.path.join(ROOT, "rustpotter_amd", "csrc", "Makefile")).read()
    for src in sorted({s for s, _ in KERNELS.values()}):
        assert src in mk, src


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_mixed_kernels_spill_nothing(remarks, kernel):
    assert kernel in remarks, sorted(remarks)
    regs, spill, scratch = remarks[kernel]
    print("%s: %d registers, %d spilled values, %d bytes of scratch" % (kernel, regs, spill, scratch))
    assert spill == 0, "%s: %d spilled values" % (kernel, spill)
    assert scratch == 0, "%s: %d bytes of scratch" % (kernel, scratch)
    assert regs <= KERNELS[kernel][1], "%s: %d registers, %d when it was written" % (kernel, regs, KERNELS[kernel][1])
