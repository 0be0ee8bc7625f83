"""tests/abandon_ref.py on CPU-checkable ground: the f64 restatement against the strict-f32 oracle, the theorem early abandon rests on
(and the trap next to it), and the exact bound against the kernels' own."""
import numpy as np
import pytest

import abandon_ref as ar
from oracle import rp_oracle as orc

K, SCORE_REF = 5, 0.22


def test_f64_restatement_agrees_with_the_oracle():
    """Random frames, templates of unequal lengths, bands 3..7: within f32 rounding of orc.score_stream (catches an off-by-one in the band or
    the read-out cell) -- for one stream and for the several-streams form the GPU tests use."""
    rng = np.random.default_rng(7)
    mf = rng.standard_normal((2, 150, K)).astype(np.float32) * 3 + 1
    templates = [(rng.standard_normal((n, K)) * 2).astype(np.float32) for n in (40, 57, 33)]
    for band in (3, 4, 5, 6, 7):
        ref = np.stack([orc.score_stream(mf[s], templates, band, SCORE_REF)[0] for s in range(2)])   # [S][n_win][T], windows of the longest
        n_win = ref.shape[1]
        assert n_win == 150 - 57 + 1
        nc, tru = ar.f64_nc_scores(mf, templates, band, SCORE_REF)
        assert tru.shape == (2 * n_win, 3) and np.array_equal(tru, ar.logistic(nc, SCORE_REF))
        assert np.allclose(tru.reshape(2, n_win, 3), ref, rtol=3e-6, atol=0), band
        one = ar.f64_nc_scores(mf[1], templates, band, SCORE_REF)[1]
        assert np.array_equal(one, tru[n_win:])
        assert np.array_equal(ar.f64_scores(mf[0], templates[:1], band, SCORE_REF)[:n_win, 0], tru[:n_win, 0])


def _band_min(D, axis_rows, i):
    return (D[:, i, 1:] if axis_rows else D[:, 1:, i]).min(axis=1)


@pytest.mark.parametrize("band", [3, 4, 5, 6])
def test_every_row_and_column_bounds_the_read_out_cell(band):
    """The theorem the kernels rest on, in f64 on random frames: the cheapest band cell of every row r <= m-1 and of every column c <= n is a
    lower bound of D[m-1][n] (costs are >= 0; a warping path to (m-1, n) crosses them all)."""
    rng = np.random.default_rng(100 + band)
    mf = rng.standard_normal((90, K)).astype(np.float32) * 2 + 0.5
    for m in (2 * band + 1, 2 * band + 2, 25, 36):
        tpl = (rng.standard_normal((m, K)) * 2).astype(np.float32)
        D = ar.f64_dtw(mf, tpl, band)
        end = D[:, m - 1, m]
        assert np.isfinite(end).all() and (end > 0).all()
        for r in range(1, m):
            assert (_band_min(D, True, r) <= end).all(), (m, r)
        for c in range(1, m + 1):
            assert (D[:, 1:m, c].min(axis=1) <= end).all(), (m, c)       # rows 1 .. m-1 of the column
            assert (_band_min(D, False, c) <= end).all(), (m, c)         # a kernel that also looks at row m only lowers the minimum


def test_row_m_is_not_a_lower_bound():
    """The trap: the read-out cell lies in row m-1, so a check placed one row late is unsound.  Window (-2u, u, u) -- centred as it stands --
    against the template (-u, u, v) with v at a right angle to u: rows 1 and 2 match columns 1 and 2..3 exactly, D[m-1][n] = 0, while every
    cell of row m costs 1."""
    u, v = np.zeros(K, np.float32), np.zeros(K, np.float32)
    u[0], v[1] = 1.0, 1.0
    win = np.stack([-2 * u, u, u])
    tpl = np.stack([-u, u, v])
    m = n = 3
    D = ar.f64_dtw(win, tpl, 3)[0]
    assert D[m - 1, n] == 0.0
    assert D[m, 1:].min() == 1.0                    # > D[m-1][n]: row m's band minimum says "past the bound" of a DTW whose score is the best there is
    for r in range(1, m):
        assert D[r, 1:].min() <= D[m - 1, n]
    for c in range(1, n + 1):
        assert D[1:m, c].min() <= D[m - 1, n]
    assert ar.logistic(D[m - 1, n] / (m + n), 0.22) > 0.73 > ar.logistic(D[m, 1:].min() / (m + n), 0.22)


def test_nc_max_inverts_the_logistic_and_the_kernels_bound_is_larger():
    """score(nc_max) == threshold to 1e-12, and dtw_abandon_nc's margin (x 1.001 + 1e-4, evaluated in f32 as the launcher does) keeps the
    kernels' bound strictly above the exact one for thresholds all over (0, 1) -- the threshold a kernel is handed is an f32, so the exact
    bound is taken of that value.  Where the exact bound is positive (threshold < 1 / (1 + 1/e): a DTW can be above it at all) the f32
    logarithm costs the margin next to nothing; near 1 the rounding of 1 / threshold - 1 eats into it but never through it."""
    rng = np.random.default_rng(11)
    grid = np.concatenate([np.linspace(0.001, 0.999, 999), [1e-30, 1e-6, 0.5, 0.9, 0.99, 0.999, 0.9999, 1 - 1e-6, 1 - 2.0 ** -24],
                           rng.uniform(0.999, 1.0, 2000), rng.uniform(0.0, 1.0, 2000)])
    thresholds = np.unique(grid.astype(np.float32))
    thresholds = thresholds[(thresholds > 0) & (thresholds < 1)].astype(np.float64)
    assert thresholds.size > 4000
    for score_ref in (0.05, 0.1, 0.22, 0.3):
        b = ar.nc_max(thresholds, score_ref)
        assert np.abs(ar.logistic(b, score_ref) - thresholds).max() <= 1e-12
        # strictly decreasing in the threshold; negative once threshold > 1 / (1 + 1/e) = 0.731..
        assert (np.diff(b) < 0).all() and (b[thresholds > 0.7311] < 0).all() and (b[thresholds < 0.731] > 0).all()
        for thr, exact in zip(thresholds, b):
            k = float(ar.kernel_abandon_nc(thr, score_ref))
            assert k > exact, (thr, score_ref, k, exact)
            if exact >= 0:
                assert k - exact >= 0.99e-4 + 0.99e-3 * exact, (thr, score_ref, k - exact)


def test_reference_detections_is_scan_ref_per_stream():
    from scan_ref import scan_ref
    rng = np.random.default_rng(3)
    agg = rng.random((3, 80)) * 0.6
    agg[1, 30:34] = (0.7, 0.9, 0.8, 0.75)
    avg = rng.random((3, 80))
    got = ar.reference_detections(agg, 80 + 19, 20, 0.65, 2)
    assert [len(g) for g in got] == [0, 1, 0] and got[1][0][1:3] == (31, 4) and got[1][0][4] == np.float32(0.9)
    for s in range(3):
        assert got[s] == scan_ref(agg[s], None, 99, 20, 0.65, 0.0, 2, False, None, 0.0)
    gated = ar.reference_detections(agg, 99, 20, 0.65, 1, avg=avg, avg_threshold=0.5)
    for s in range(3):
        assert gated[s] == scan_ref(agg[s], avg[s], 99, 20, 0.65, 0.5, 1, False, None, 0.0)
