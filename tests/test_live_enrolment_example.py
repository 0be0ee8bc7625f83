"""examples/live_enrolment.c: an empty reserved bank, a live batch over it, a wakeword enrolled from the golden recordings while the batch
runs, the slot connected, a detection.  The program compiles as C99 without warnings and links against the shared library (CPU); on the
GPU it runs and reports the detection."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "live_enrolment")
    lib_dir = os.path.join(ROOT, "rustpotter_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "live_enrolment.c"),
           "-L" + lib_dir, "-lrustpotter_hip", "-Wl,-rpath," + lib_dir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_live_enrolment_example_compiles_and_links(tmp_path):
    import rustpotter_amd
    rustpotter_amd.load_library()   # the library the program links against is built
    build(tmp_path)


@pytest.mark.gpu
def test_live_enrolment_example_detects(tmp_path):
    g = os.path.join(ROOT, "tests", "golden")
    exe = build(tmp_path)
    r = subprocess.run([exe] + [os.path.join(g, "oye_casa_g_%d.wav" % i) for i in range(1, 6)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 wakeword(s) in the bank, 0 detection(s) so far" in r.stdout and "enrolled wakeword 0: windows of " in r.stdout, r.stdout
    assert "slot 1: detection at chunk " in r.stdout and "1 wakeword(s) in the bank, " in r.stdout, r.stdout
    assert "slot 0:" not in r.stdout and "slot 2:" not in r.stdout and "slot 3:" not in r.stdout, r.stdout
