"""Child processes for launch switches that the library reads once per process (RP_MFCC_BLOCKS, RP_FRONTEND_TILE, ...): one script, one
fresh Python process per setting, one at a time, each under its own timeout.  The first child that does not return 0 -- or does not
return in time -- fails the test with its output, and no further child is started after it."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")

# what a child starts with: the package and the test helpers on the path, one context with host pointers
PRELUDE = """import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import rustpotter_amd as ra
ctx = ra.BatchContext(device=0, host_pointers=True)
""" % (ROOT, TESTS)


def run_each(tmp_path, body, settings, timeout):
    """body: the script after PRELUDE; it saves its arrays with np.savez(sys.argv[1], ...).  settings: [(name, {variable: value})].
    -> {name: the child's arrays}.  timeout: seconds a child may take (it imports the package, opens the device and runs for seconds)."""
    script = tmp_path / "child.py"
    script.write_text(PRELUDE + body)
    results = {}
    for name, extra in settings:
        out = tmp_path / ("%s.npz" % name)
        try:
            r = subprocess.run([sys.executable, str(script), str(out)], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **extra))
        except subprocess.TimeoutExpired as e:
            pytest.fail("child %s %r did not return within %d s; no further child is started\n%s\n%s" % (name, extra, timeout, e.stdout, e.stderr))
        if r.returncode != 0:
            pytest.fail("child %s %r returned %d; no further child is started\n%s\n%s" % (name, extra, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
        with np.load(str(out)) as z:
            results[name] = {k: z[k] for k in z.files}
    return results
