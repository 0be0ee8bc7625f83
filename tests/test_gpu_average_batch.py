"""rp_mfcc_average_batch: MfccAverager::average (src/mfcc/averager.rs:5-37) for many wakewords per call, on the device
(rustpotter_amd/csrc/rp_average.hip), against the reference's own files and against the oracle's fold (orc_average_step, which
reproduces the reference's avg_features bit for bit: tests/test_oracle_golden.py G3).  The kernel restates the host arithmetic
operation for operation, so every comparison is np.array_equal: no tolerance."""
import os

import numpy as np
import pytest

import rpw_py
import simstream
from oracle import rp_oracle as orc

pytestmark = pytest.mark.gpu

G = simstream.GOLDEN


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


def oracle_fold(templates):
    """MfccAverager::average over templates in the GIVEN order: the first is the origin, orc_average_step folds the others in."""
    origin = np.ascontiguousarray(templates[0], np.float32).copy()
    for fr in templates[1:]:
        fr = np.ascontiguousarray(fr, np.float32)
        orc.lib().orc_average_step(orc._f(origin), origin.shape[0], orc._f(fr), fr.shape[0], origin.shape[1])
    return origin


def check_call(ctx, wakewords):
    got = ctx.average_templates(wakewords)
    assert len(got) == len(wakewords)
    bad = []
    for w, (g, ww) in enumerate(zip(got, wakewords)):
        ref = oracle_fold(ww)
        assert g.shape == ref.shape and g.dtype == np.float32
        assert np.all(np.isfinite(ref)), "the case itself must stay finite"
        if not np.array_equal(g, ref):
            bad.append((w, [t.shape[0] for t in ww], float(np.abs(g - ref).max())))
    assert not bad, "wakewords that differ from the oracle (index, lengths, max |d|): %s" % bad[:8]


def builder_order(named):
    """compute_avg_samples_features' fold order (wakeword_ref_build.rs:90-110): longest first, equal lengths by name"""
    return [v for _, v in sorted(named.items(), key=lambda kv: (-len(kv[1]), kv[0]))]


def test_reference_files_in_one_call(ctx):
    """samples_features of three .rpw files the reference wrote (5, 3 and 6 templates), one call: each result is that file's avg_features."""
    files = [rpw_py.load_rpw(os.path.join(G, f)) for f in ("oye_casa_g.rpw", "alexa.rpw", "oye_casa_real.rpw")]
    assert [len(f["samples_features"]) for f in files] == [5, 3, 6]
    got = ctx.average_templates([builder_order(f["samples_features"]) for f in files])
    for g, f in zip(got, files):
        assert g.shape == f["avg_features"].shape
        assert np.array_equal(g, f["avg_features"])


PAIRS = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (9, 5), (64, 65), (65, 64), (100, 93)]


@pytest.mark.parametrize("K", [1, 3, 5, 13, 16, 23])
def test_edge_shapes(ctx, K):
    """One call per K: every (origin, frames) pair of PAIRS as a wakeword of two templates, then wakewords of 1..9 templates whose lengths
    are neither sorted nor equal (folds with fewer origin rows than frames among them)."""
    rng = np.random.default_rng(1000 + K)
    wakewords = [[rng.standard_normal((m, K)).astype(np.float32), rng.standard_normal((n, K)).astype(np.float32)] for m, n in PAIRS]
    for count in range(1, 10):
        lens = rng.permutation(np.arange(3, 41))[:count]   # distinct, unsorted
        wakewords.append([(2.5 * rng.standard_normal((int(n), K))).astype(np.float32) for n in lens])
    assert any(ww[0].shape[0] < max(t.shape[0] for t in ww[1:]) for ww in wakewords if len(ww) > 2)
    check_call(ctx, wakewords)


def test_ties_and_zero_norms(ctx):
    """mfcc_size 1 with rows of +-1: every cost is exactly 0 or 2, so the back-trace is decided by the ORDER of its three comparisons;
    identical templates; all-zero rows and an all-zero template (magnitude 0: the cost is 1 - 0)."""
    rng = np.random.default_rng(7)
    pm1 = lambda n: rng.choice(np.array([-1.0, 1.0], np.float32), size=(n, 1))
    wakewords = [[pm1(int(n)) for n in rng.integers(1, 30, size=int(c))] for c in (2, 3, 5, 8, 2, 4)]
    one = pm1(12)
    wakewords.append([one.copy(), one.copy(), one.copy()])
    check_call(ctx, wakewords)
    K = 5
    zr = []
    for c in (2, 4, 3):
        ts = []
        for n in rng.integers(4, 25, size=c):
            t = rng.standard_normal((int(n), K)).astype(np.float32)
            t[rng.random(int(n)) < 0.3] = 0.0
            ts.append(t)
        zr.append(ts)
    same = rng.standard_normal((17, K)).astype(np.float32)
    zr.append([same.copy() for _ in range(4)])
    zr.append([rng.standard_normal((9, K)).astype(np.float32), np.zeros((11, K), np.float32), rng.standard_normal((6, K)).astype(np.float32)])
    zr.append([np.zeros((8, K), np.float32), rng.standard_normal((10, K)).astype(np.float32)])
    zr.append([np.zeros((5, K), np.float32), np.zeros((7, K), np.float32)])
    check_call(ctx, zr)


def test_matrix_in_workspace_and_in_lds(ctx):
    """230 x 215 x 4 bytes = 198 KB does not fit a CU's 160 KB of LDS: that wakeword's cost matrix lives in the context's workspace;
    the 40 x 37 wakewords of the same call keep theirs in LDS."""
    rng = np.random.default_rng(4)
    K = 16
    small = lambda: [rng.standard_normal((40, K)).astype(np.float32), rng.standard_normal((37, K)).astype(np.float32)]
    big = [rng.standard_normal((n, K)).astype(np.float32) for n in (230, 215, 190)]
    check_call(ctx, [small(), big, small(), small()])


def test_more_wakewords_than_the_device_holds(ctx):
    rng = np.random.default_rng(5)
    K = 5
    wakewords = [[rng.standard_normal((int(n), K)).astype(np.float32) for n in rng.integers(20, 61, size=int(c))]
                 for c in rng.integers(2, 7, size=600)]
    check_call(ctx, wakewords)


def test_refusals(ra, ctx):
    """an empty call is a success; a wakeword without templates or a template without rows is refused, and the context works afterwards"""
    assert ctx.average_templates([]) == []
    t = np.ones((3, 5), np.float32)
    with pytest.raises(ra.RustpotterError, match="at least one template"):
        ctx.average_templates([[t], []])
    with pytest.raises(ra.RustpotterError, match="without frames"):
        ctx.average_templates([[t, np.zeros((0, 5), np.float32)]])
    got = ctx.average_templates([[t]])
    assert np.array_equal(got[0], t)
