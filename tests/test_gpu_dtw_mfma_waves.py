"""The two builds of the three-part eight-slot dtw_mfma_kernel (rustpotter_amd/csrc/rp_dtw_mfma.hip): twelve waves per workgroup
(three per SIMD, 168 registers: the default where twelve waves' frame stages fit) and eight (RP_MFMA3_WAVES=8).  They differ in registers and
scheduling only -- the twelve-wave build reads two tiles' second-step operand from LDS where the other holds it, and splits a frame in two
pieces where the other takes four -- so both must answer the bits recorded in tests/golden/dtw_mfma_operand.npz.
tests/test_gpu_dtw_mfma_operand.py holds whichever build is the default to that fixture; this test pins the other one too.  The variable is
read once per process: each build runs in a child process of its own, one after the other; a child that fails ends the test."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(TESTS, "golden", "dtw_mfma_operand.npz")
# 3 streams x 45 windows: tiles straddle streams, the guarded block alone (12), an odd tail (13, 17, 25), the zero-vector window and the
# out-of-range frame (25: the fix list), bands 3 and 4, and the four-slot shape (17 x 4: twelve waves in either child)
NAMES = ["L12_T8", "L13_T8", "L25_T8", "band3_L13_T5", "band4_L24_T7", "L17_T4"]

CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import rustpotter_amd as ra
import test_gpu_dtw_mfma_operand as op
names, out_path = sys.argv[1].split(","), sys.argv[2]
with np.load(op.GOLDEN) as z:
    golden = {k: z[k] for k in z.files}
ctx = ra.BatchContext(device=0, host_pointers=True, arithmetic="f32_matrix")
out = {}
for name in names:
    scores, agg, listed = op._run_staged(ra, ctx, op.STAGED[name][0], golden[name + "/templates"], golden[name + "/mfcc"])
    assert ctx.last_dtw_products == ["bf16x3"], ctx.last_dtw_products
    # the build that ran: the eight-slot cases follow the variable, the four-slot one (L17_T4) runs twelve waves whatever it says
    assert ctx.last_dtw_mfma_waves == [12 if op.STAGED[name][2] <= 4 else int(sys.argv[3])], (name, ctx.last_dtw_mfma_waves)
    out[name + "/scores"], out[name + "/agg"], out[name + "/listed"] = scores, agg, listed
np.savez(out_path, **out)
"""


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_eight_and_twelve_wave_builds_give_the_recorded_bits(tmp_path):
    with np.load(GOLDEN) as z:
        golden = {k: z[k] for k in z.files}
    script = tmp_path / "waves_child.py"
    script.write_text(CHILD % {"root": os.path.dirname(TESTS), "tests": TESTS})
    for nw in ("8", "12"):
        env = dict(os.environ)
        env["RP_MFMA3_WAVES"] = nw
        out_path = str(tmp_path / ("waves_%s.npz" % nw))
        r = subprocess.run([sys.executable, str(script), ",".join(NAMES), out_path, nw], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, "RP_MFMA3_WAVES=%s: %s" % (nw, r.stdout[-1000:] + r.stderr[-2000:])
        with np.load(out_path) as z:
            got = {k: z[k] for k in z.files}
        for name in NAMES:
            want_scores, want_agg = golden["f32_matrix/%s/scores" % name], golden["f32_matrix/%s/agg" % name]
            want_listed = int(golden["f32_matrix/%s/listed" % name])
            where = "RP_MFMA3_WAVES=%s, %s" % (nw, name)
            assert got[name + "/scores"].shape == want_scores.shape, where
            assert int(got[name + "/listed"]) == want_listed, (where, int(got[name + "/listed"]), want_listed)
            assert np.array_equal(_bits(got[name + "/scores"]), _bits(want_scores)), (where, int((_bits(got[name + "/scores"]) != _bits(want_scores)).sum()))
            assert np.array_equal(_bits(got[name + "/agg"]), _bits(want_agg)), where
        assert int(golden["f32_matrix/L25_T8/listed"]) > 0
