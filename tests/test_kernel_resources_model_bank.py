"""mlp_windows_bank_kernel (rustpotter_amd/csrc/rp_mlp_windows.hip), the model bank's forward: every build <1..7> exists, spills nothing, uses no
scratch memory and keeps the two waves per SIMD the three-part form of mlp_windows_kernel is built for (three planes of frames and up to
seven accumulator tiles).  It shares its body with mlp_windows_kernel; the model comes through the stream's descriptor and the tiles behind
the stream's own are skipped by run-time tests -- an accumulator array the compiler indexes at run time would go to scratch memory, and
exactly these counters show it.  The register counts the build gave when the kernel was written are caps.  The compiler's occupancy
figure follows the registers: 2 for <5>, <6> and <7>, the builds that fill the budget, 3 to 5 for the smaller ones -- the test asks for the
two waves per SIMD the kernel is built for, or more.  Reads the compiler's own
resource remarks (tools/kernel_regs.py compiles with the Makefile's flags; CPU only, hipcc cross-compiles), as
tests/test_kernel_resources_bank.py does."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> registers of the build the kernel was written with
KERNELS = {
    "mlp_windows_bank_kernel<1>": 94, "mlp_windows_bank_kernel<2>": 121, "mlp_windows_bank_kernel<3>": 137, "mlp_windows_bank_kernel<4>": 153,
    "mlp_windows_bank_kernel<5>": 182, "mlp_windows_bank_kernel<6>": 186, "mlp_windows_bank_kernel<7>": 202,
}


@pytest.fixture(scope="module")
def remarks():
    out = {}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "rp_mlp_windows.hip", "mlp_windows_bank_kernel"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    for line in r.stdout.splitlines()[1:]:
        f = line.split(None, 7)   # vgpr agpr spill sgpr scrtch lds occ name
        if len(f) == 8:
            out[re.sub(r"^(void )?rp::", "", f[7]).strip()] = (int(f[0]) + int(f[1]), int(f[2]), int(f[4]), int(f[6]))
    return out


def test_every_instantiation_is_listed(remarks):
    """one build per tile count a workgroup can own, 1 .. 7 (kWinMaxTiles)"""
    assert sorted(remarks) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_bank_kernel_spills_nothing_at_two_waves(remarks, kernel):
    assert kernel in remarks, sorted(remarks)
    regs, spill, scratch, occ = remarks[kernel]
    print("%s: %d registers, %d spilled values, %d bytes of scratch, %d waves per SIMD" % (kernel, regs, spill, scratch, occ))
    assert spill == 0, "%s: %d spilled values" % (kernel, spill)
    assert scratch == 0, "%s: %d bytes of scratch" % (kernel, scratch)
    assert occ >= 2, "%s: %d waves per SIMD" % (kernel, occ)
    assert regs <= KERNELS[kernel], "%s: %d registers, %d when it was written" % (kernel, regs, KERNELS[kernel])
