"""The per-stream forms of the gain-normaliser kernels (rustpotter_amd/csrc/rp_frontend.hip: gain_per_stream_kernel for
rp_frontend_batch_bank, stream_filters_kernel<..., PER = true> for rp_stream_batch_set_filters_bank) against the shared-wakeword forms they
were derived from: nothing spilled, no scratch memory, an LDS tile no larger than the shared form's, and the register count (vector +
accumulation registers) of the build they were written with as a cap.  The shared forms -- gain_kernel and every stream_filters_kernel
instantiation with PER = false -- must report exactly the registers, LDS and scratch they had before the per-stream flag existed: the numbers
below were read with the same tool from the commit before it.  Reads the compiler's own resource remarks (tools/kernel_regs.py compiles with
the Makefile's flags; CPU only, hipcc cross-compiles), as tests/test_kernel_resources_stream_bank.py does."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ("float", "int", "short", "signed char")
# (registers, LDS bytes) of stream_filters_kernel<TIN, VEC, GAIN, BP> before the PER flag, by (TIN, VEC) and (GAIN, BP)
SHARED_BEFORE = {}
for _t in TYPES:
    SHARED_BEFORE[(_t, "false")] = {("false", "true"): 220, ("true", "false"): 219, ("true", "true"): 223}
SHARED_BEFORE[("float", "true")] = SHARED_BEFORE[("int", "true")] = {("false", "true"): 220, ("true", "false"): 219, ("true", "true"): 223}
SHARED_BEFORE[("short", "true")] = {("false", "true"): 172, ("true", "false"): 171, ("true", "true"): 175}
SHARED_BEFORE[("signed char", "true")] = {("false", "true"): 148, ("true", "false"): 147, ("true", "true"): 151}
SHARED_LDS = 25600
GAIN_KERNEL_BEFORE = (19, 0)   # registers, LDS (its ring is dynamic LDS)
# registers of the per-stream instantiations in the build they were written with, by (TIN, VEC) and BP
PER_CAPS = {
    ("float", "false"): {"false": 221, "true": 224}, ("float", "true"): {"false": 221, "true": 224},
    ("int", "false"): {"false": 221, "true": 225}, ("int", "true"): {"false": 221, "true": 224},
    ("short", "false"): {"false": 221, "true": 225}, ("short", "true"): {"false": 173, "true": 176},
    ("signed char", "false"): {"false": 221, "true": 225}, ("signed char", "true"): {"false": 149, "true": 152},
}
GAIN_PER_STREAM_CAP = 19


@pytest.fixture(scope="module")
def remarks():
    """kernel name -> (registers, spilled values, scratch bytes, LDS bytes)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "rp_frontend.hip", "_kernel"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines()[1:]:
        f = line.split(None, 7)   # vgpr agpr spill sgpr scrtch lds occ name
        if len(f) == 8:
            out[re.sub(r"^(void )?rp::", "", f[7]).strip()] = (int(f[0]) + int(f[1]), int(f[2]), int(f[4]), int(f[5]))
    return out


def sf(t, vec, gain, bp, per):
    return "stream_filters_kernel<%s, %s, %s, %s, %s>" % (t, vec, gain, bp, per)


def test_every_stream_filters_instantiation_is_known(remarks):
    """the shared forms and the per-stream forms (gain normaliser on, with and without the band-pass) and nothing else"""
    want = {sf(t, v, g, b, "false") for t in TYPES for v in ("false", "true") for g, b in (("false", "true"), ("true", "false"), ("true", "true"))}
    want |= {sf(t, v, "true", b, "true") for t in TYPES for v in ("false", "true") for b in ("false", "true")}
    assert {k for k in remarks if k.startswith("stream_filters_kernel")} == want
    assert "gain_kernel" in remarks and "gain_per_stream_kernel" in remarks


def test_shared_forms_are_what_they_were(remarks):
    assert remarks["gain_kernel"] == (GAIN_KERNEL_BEFORE[0], 0, 0, GAIN_KERNEL_BEFORE[1])
    for (t, v), by_filters in SHARED_BEFORE.items():
        for (g, b), regs in by_filters.items():
            name = sf(t, v, g, b, "false")
            assert remarks[name] == (regs, 0, 0, SHARED_LDS), (name, remarks[name])


@pytest.mark.parametrize("tin", TYPES)
def test_per_stream_forms_spill_nothing(remarks, tin):
    for v in ("false", "true"):
        for b in ("false", "true"):
            name = sf(tin, v, "true", b, "true")
            regs, spill, scratch, lds = remarks[name]
            print("%s: %d registers, %d spilled values, %d bytes of scratch, %d bytes of LDS" % (name, regs, spill, scratch, lds))
            assert spill == 0 and scratch == 0, name
            assert lds <= remarks[sf(tin, v, "true", b, "false")][3], name
            assert regs <= PER_CAPS[(tin, v)][b], "%s: %d registers, %d when it was written" % (name, regs, PER_CAPS[(tin, v)][b])


def test_gain_per_stream_kernel(remarks):
    regs, spill, scratch, lds = remarks["gain_per_stream_kernel"]
    print("gain_per_stream_kernel: %d registers, %d spilled values, %d bytes of scratch, %d bytes of static LDS" % (regs, spill, scratch, lds))
    assert spill == 0 and scratch == 0 and lds <= remarks["gain_kernel"][3]
    assert regs <= GAIN_PER_STREAM_CAP
