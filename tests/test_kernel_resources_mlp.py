"""The kernels of the wakeword-model forward (rustpotter_amd/csrc/rp_mlp.hip, rp_mlp_windows.hip, rp_mlp_stream.hip): every build exists and
keeps the registers, the spilled values, the scratch memory and the waves per SIMD it had before the kernels' shared pieces (the operand
splits, the tail layers, the narrow staged-frame kernels' sweep and layer-1 value) moved into device functions of rp_mlp_dev.h.  A helper
whose arguments the compiler does not fold costs registers, and the staged-frame kernels sit on the steps of the occupancy table (96, 128,
168 registers); mlp_mfma_kernel<5, ..> and <9, ..> sit at the 168-register cap of their launch bounds, where more spilled values are a
slowdown.  The occupancies and the spill / scratch figures are those of the build before the move; the register counts are caps from the
build the test was written with.  Reads the compiler's own resource remarks (tools/kernel_regs.py compiles with the Makefile's flags; CPU
only, hipcc cross-compiles), as tests/test_kernel_resources_model_bank.py does for mlp_windows_bank_kernel."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mlp_windows_kernel<NT, P3>: (waves per SIMD at least, registers at most)
NARROW = {(nt, p3): (occ, regs)
          for p3, occs, regss in ((False, (6, 5, 4, 4, 3, 3, 3), (73, 94, 102, 118, 155, 154, 166)),
                                  (True, (5, 4, 4, 3, 3, 2, 2), (94, 106, 126, 142, 158, 174, 190)))
          for nt, occ, regs in zip(range(1, 8), occs, regss)}
# mlp_windows_wide_kernel<NT, NQ, P3>
WIDE = {(nt, nq, p3): (occ, regs)
        for nt, p3, occ, regss in ((2, False, 3, (132, 132, 132, 132)), (2, True, 3, (131, 131, 131, 131)),
                                   (4, False, 4, (126, 128, 126, 128)), (4, True, 3, (152, 152, 152, 152)))
        for nq, regs in zip(range(2, 6), regss)}
# mlp_mfma_kernel<NT, PREC>: (waves per SIMD at least, registers, spilled values, bytes of scratch at most)
MFMA = {
    (1, 0): (4, 124, 0, 0), (1, 1): (3, 130, 0, 0), (1, 2): (3, 136, 0, 0), (1, 5): (3, 156, 0, 0),
    (2, 0): (3, 144, 0, 0), (2, 1): (3, 130, 0, 0), (2, 2): (3, 160, 0, 0), (2, 5): (3, 156, 0, 0),
    (5, 0): (3, 168, 10, 44), (5, 1): (3, 168, 0, 0), (5, 2): (3, 168, 16, 28), (5, 5): (3, 168, 111, 152),
    (9, 0): (3, 168, 181, 312), (9, 1): (3, 168, 35, 64), (9, 2): (3, 168, 168, 236), (9, 5): (3, 168, 352, 500),
}
# mlp_stream_kernel<NT, PREC, D, waves>, per (NT, PREC): (waves per SIMD at least, registers at most); D, waves = (1, 4), (1, 8), (2, 6), (2, 8)
STREAM = {(1, 0): (4, 126), (1, 1): (4, 122), (1, 2): (4, 127), (1, 5): (3, 131), (2, 0): (3, 133), (2, 1): (4, 125), (2, 2): (3, 134), (2, 5): (3, 151)}
STREAM_RINGS = ((1, 4), (1, 8), (2, 6), (2, 8))


def _remarks(source, name):
    """kernel (template arguments as the compiler prints them) -> (registers, spilled values, bytes of scratch, waves per SIMD)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), source, name], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines()[1:]:
        f = line.split(None, 7)   # vgpr agpr spill sgpr scrtch lds occ name
        if len(f) == 8:
            out[re.sub(r"^(void )?rp::", "", f[7]).strip()] = (int(f[0]) + int(f[1]), int(f[2]), int(f[4]), int(f[6]))
    return out


@pytest.fixture(scope="module")
def windows():
    return _remarks("rp_mlp_windows.hip", "mlp_windows_")


@pytest.fixture(scope="module")
def mfma():
    return _remarks("rp_mlp.hip", "mlp_mfma_kernel")


@pytest.fixture(scope="module")
def stream():
    return _remarks("rp_mlp_stream.hip", "mlp_stream_kernel")


def _b(v):
    return "true" if v else "false"


def _check(remarks, kernel, occ_min, regs_max, spill_max=0, scratch_max=0):
    assert kernel in remarks, sorted(remarks)
    regs, spill, scratch, occ = remarks[kernel]
    print("%s: %d registers, %d spilled values, %d bytes of scratch, %d waves per SIMD" % (kernel, regs, spill, scratch, occ))
    assert spill <= spill_max, "%s: %d spilled values, %d before" % (kernel, spill, spill_max)
    assert scratch <= scratch_max, "%s: %d bytes of scratch, %d before" % (kernel, scratch, scratch_max)
    assert occ >= occ_min, "%s: %d waves per SIMD, %d before" % (kernel, occ, occ_min)
    assert regs <= regs_max, "%s: %d registers, %d when the test was written" % (kernel, regs, regs_max)


def test_every_staged_frame_build_is_listed(windows):
    """mlp_windows_kernel<1..7, P3>, mlp_windows_wide_kernel<{2, 4}, 2..5, P3> and the bank kernel's seven builds, nothing else"""
    want = ["mlp_windows_kernel<%d, %s>" % (nt, _b(p3)) for nt, p3 in NARROW]
    want += ["mlp_windows_wide_kernel<%d, %d, %s>" % (nt, nq, _b(p3)) for nt, nq, p3 in WIDE]
    want += ["mlp_windows_bank_kernel<%d>" % nt for nt in range(1, 8)]
    assert sorted(windows) == sorted(want)


@pytest.mark.parametrize("nt,p3", sorted(NARROW))
def test_windows_kernel_spills_nothing_and_keeps_its_waves(windows, nt, p3):
    _check(windows, "mlp_windows_kernel<%d, %s>" % (nt, _b(p3)), *NARROW[nt, p3])


@pytest.mark.parametrize("nt,nq,p3", sorted(WIDE))
def test_windows_wide_kernel_spills_nothing_and_keeps_its_waves(windows, nt, nq, p3):
    _check(windows, "mlp_windows_wide_kernel<%d, %d, %s>" % (nt, nq, _b(p3)), *WIDE[nt, nq, p3])


def test_every_mfma_and_stream_build_is_listed(mfma, stream):
    assert sorted(mfma) == sorted("mlp_mfma_kernel<%d, %d>" % k for k in MFMA)
    assert sorted(stream) == sorted("mlp_stream_kernel<%d, %d, %d, %d>" % (k + ring) for k in STREAM for ring in STREAM_RINGS)


@pytest.mark.parametrize("nt,prec", sorted(MFMA))
def test_mfma_kernel_keeps_three_waves_and_spills_no_more(mfma, nt, prec):
    _check(mfma, "mlp_mfma_kernel<%d, %d>" % (nt, prec), *MFMA[nt, prec])


@pytest.mark.parametrize("nt,prec", sorted(STREAM))
def test_stream_kernel_spills_nothing_and_keeps_its_waves(stream, nt, prec):
    for ring in STREAM_RINGS:
        _check(stream, "mlp_stream_kernel<%d, %d, %d, %d>" % ((nt, prec) + ring), *STREAM[nt, prec])
