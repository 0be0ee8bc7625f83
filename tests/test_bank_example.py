"""examples/personal_wakewords.c: the wakeword bank from plain C99 -- two golden .rpw files in one bank, two streams with different
wakeword indices.  Builds with -Wall -Wextra -Werror against the shared library (CPU); on the GPU it must print the reference's own
detection for oye_casa_g_1.wav (tests/detector.rs:24-37)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def build(tmp_path):
    exe = str(tmp_path / "personal_wakewords")
    lib_dir = os.path.join(ROOT, "rustpotter_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "personal_wakewords.c"),
           "-L" + lib_dir, "-lrustpotter_hip", "-Wl,-rpath," + lib_dir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_personal_wakewords_example_builds(tmp_path):
    build(tmp_path)


@pytest.mark.gpu
def test_personal_wakewords_example_runs(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe] + [os.path.join(G, n) for n in ("oye_casa_g.rpw", "alexa.rpw", "oye_casa_g_1.wav", "alexa.wav")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wakeword 0: windows of 108 frames" in r.stdout and "wakeword 1: windows of 126 frames" in r.stdout, r.stdout
    assert "stream 0 (wakeword 0): 1 detection(s)" in r.stdout and "score 0.7310586 avg_score 0.6495044" in r.stdout, r.stdout
    assert "stream 1 (wakeword 1):" in r.stdout, r.stdout
