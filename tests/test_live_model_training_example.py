"""examples/live_model_training.c: an empty reserved model bank, a live batch over it, two models trained from the golden recordings into
the bank while the batch runs, their slots connected, the next audio run through them.  The program compiles as C99 without warnings and
links against the shared library (CPU); on the GPU it runs and reports the bank's growth from 0 to 2 models under the batch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "live_model_training")
    lib_dir = os.path.join(ROOT, "rustpotter_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "live_model_training.c"),
           "-L" + lib_dir, "-lrustpotter_hip", "-Wl,-rpath," + lib_dir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_live_model_training_example_compiles_and_links(tmp_path):
    import rustpotter_amd
    rustpotter_amd.load_library()   # the library the program links against is built
    build(tmp_path)


@pytest.mark.gpu
def test_live_model_training_example_runs(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "0 model(s) in the bank, 0 detection(s) so far" in r.stdout, r.stdout
    # the golden training set gives windows of 168 frames (tests/golden/expectations.json, "train_size") and the labels none / oye casa
    assert "trained model 0: windows of 168 frames, 2 labels, loss " in r.stdout and "trained model 1: windows of " in r.stdout, r.stdout
    # one pool replacement: the reservation's own, whose hints then held through the training
    assert re.search(r"2 model\(s\) in the bank, \d+ detection\(s\), 1 pool growth\(s\)", r.stdout), r.stdout
    assert "slot 0:" not in r.stdout and "slot 3:" not in r.stdout, r.stdout   # nobody connected there
    for line in r.stdout.splitlines():
        m = re.match(r"slot (\d): detection at chunk \d+ by model (\d), label (\d),", line)
        if m:
            assert int(m.group(2)) == int(m.group(1)) - 1 and m.group(3) == "1", line   # each slot its own model; label 0 is "none"
