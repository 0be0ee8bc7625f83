"""The kernels of model sets (rustpotter_amd/csrc/rp_mlp_model_set.hip, and their scan kernels in rp_scan_sets.hip): every instantiation is listed, spills
nothing, uses no scratch memory and keeps the waves per SIMD the file header states -- mlp_set_stream_kernel<1> three (at most 168
registers), <2> two, mlp_windows_model_set_kernel<1 .. 7> two (two workgroups of 256 threads per CU, as mlp_windows_bank_kernel, whose
body it shares).  The register counts of the build the kernels were written with are caps.  Reads the compiler's own resource remarks
(tools/kernel_regs.py compiles with the Makefile's flags; CPU only, hipcc cross-compiles), as
tests/test_kernel_resources_stream_model_bank.py does."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> (source, registers of the build the kernel was written with, waves per SIMD it is built for)
KERNELS = {
    "mlp_set_stream_kernel<1>": ("rp_mlp_model_set.hip", 132, 3), "mlp_set_stream_kernel<2>": ("rp_mlp_model_set.hip", 173, 2),
    "mlp_windows_model_set_kernel<1>": ("rp_mlp_model_set.hip", 94, 2), "mlp_windows_model_set_kernel<2>": ("rp_mlp_model_set.hip", 121, 2),
    "mlp_windows_model_set_kernel<3>": ("rp_mlp_model_set.hip", 137, 2), "mlp_windows_model_set_kernel<4>": ("rp_mlp_model_set.hip", 153, 2),
    "mlp_windows_model_set_kernel<5>": ("rp_mlp_model_set.hip", 180, 2), "mlp_windows_model_set_kernel<6>": ("rp_mlp_model_set.hip", 186, 2),
    "mlp_windows_model_set_kernel<7>": ("rp_mlp_model_set.hip", 202, 2),
    "window_means_model_set_kernel": ("rp_mlp_model_set.hip", 40, 2), "window_means_set_stream_kernel": ("rp_mlp_model_set.hip", 40, 2),
    "nn_score_model_set_kernel": ("rp_mlp_model_set.hip", 28, 2), "nn_score_set_stream_kernel": ("rp_mlp_model_set.hip", 15, 2),
    "scan_model_set_kernel": ("rp_scan_sets.hip", 91, 1), "scan_model_set_stream_kernel": ("rp_scan_sets.hip", 142, 1),
}


@pytest.fixture(scope="module")
def remarks():
    out = {}
    for src in sorted({k[0] for k in KERNELS.values()}):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), src, "_kernel"], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        for line in r.stdout.splitlines()[1:]:
            f = line.split(None, 7)   # vgpr agpr spill sgpr scrtch lds occ name
            if len(f) == 8:
                out[re.sub(r"^(void )?rp::", "", f[7]).strip()] = (int(f[0]) + int(f[1]), int(f[2]), int(f[4]), int(f[6]))
    return out


def test_every_instantiation_is_listed(remarks):
    """both row-tile builds of the live forward, one build per tile count of the whole-recording forward, and every other kernel of the
    two sources -- rp_scan_sets.hip also holds the scan kernels of wakeword sets and mixed sets, listed in the tests of their families; no
    name contains mlp_bank_stream_kernel or mlp_windows_bank_kernel, whose own tests list their instantiations"""
    import test_kernel_resources_mixed as mixed
    import test_kernel_resources_sets as sets
    sources = {k[0] for k in KERNELS.values()}
    elsewhere = {k for t in (mixed, sets) for k, v in t.KERNELS.items() if v[0] in sources}
    assert not elsewhere & set(KERNELS)
    assert sorted(remarks) == sorted(set(KERNELS) | elsewhere)
    assert not [k for k in remarks if "mlp_bank_stream_kernel" in k or "mlp_windows_bank_kernel" in k]


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_kernel_spills_nothing_at_its_waves(remarks, kernel):
    assert kernel in remarks, sorted(remarks)
    regs, spill, scratch, occ = remarks[kernel]
    _, cap, waves = KERNELS[kernel]
    print("%s: %d registers, %d spilled values, %d bytes of scratch, %d waves per SIMD" % (kernel, regs, spill, scratch, occ))
    assert spill == 0, "%s: %d spilled values" % (kernel, spill)
    assert scratch == 0, "%s: %d bytes of scratch" % (kernel, scratch)
    assert occ >= waves, "%s: %d waves per SIMD, built for %d" % (kernel, occ, waves)
    assert regs <= cap, "%s: %d registers, %d when it was written" % (kernel, regs, cap)
