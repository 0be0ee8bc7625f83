"""mlp_bank_stream_kernel (rustpotter_amd/csrc/rp_mlp_bank_stream.hip), the forward of a live-stream batch over a model bank: both builds
exist -- <1>: one 16-row tile of new windows per wave, <2>: two --, spill nothing, use no scratch memory and keep the waves per SIMD the file
header says they are built for: three for <1> (at most 168 registers), two for <2>, whose two k-blocks in flight and the one at the matrix
instructions are 3 x 40 registers of operands.  The operand queues are register arrays indexed inside unrolled loops and skipped by
wave-uniform tests; an array the compiler indexes at run time would go to scratch memory, and exactly these counters show it.  The register
counts the build gave when the kernel was written are caps.  Reads the compiler's own resource remarks (tools/kernel_regs.py compiles with
the Makefile's flags; CPU only, hipcc cross-compiles), as tests/test_kernel_resources_model_bank.py does."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> (registers of the build the kernel was written with, waves per SIMD it is built for)
KERNELS = {"mlp_bank_stream_kernel<1>": (132, 3), "mlp_bank_stream_kernel<2>": (173, 2)}


@pytest.fixture(scope="module")
def remarks():
    out = {}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "rp_mlp_bank_stream.hip", "mlp_bank_stream_kernel"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    for line in r.stdout.splitlines()[1:]:
        f = line.split(None, 7)   # vgpr agpr spill sgpr scrtch lds occ name
        if len(f) == 8:
            out[re.sub(r"^(void )?rp::", "", f[7]).strip()] = (int(f[0]) + int(f[1]), int(f[2]), int(f[4]), int(f[6]))
    return out


def test_every_instantiation_is_listed(remarks):
    """one build per number of 16-row tiles a wave owns, 1 and 2"""
    assert sorted(remarks) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_kernel_spills_nothing_at_its_waves(remarks, kernel):
    assert kernel in remarks, sorted(remarks)
    regs, spill, scratch, occ = remarks[kernel]
    cap, waves = KERNELS[kernel]
    print("%s: %d registers, %d spilled values, %d bytes of scratch, %d waves per SIMD" % (kernel, regs, spill, scratch, occ))
    assert spill == 0, "%s: %d spilled values" % (kernel, spill)
    assert scratch == 0, "%s: %d bytes of scratch" % (kernel, scratch)
    assert occ >= waves, "%s: %d waves per SIMD, built for %d" % (kernel, occ, waves)
    assert regs <= cap, "%s: %d registers, %d when it was written" % (kernel, regs, cap)
