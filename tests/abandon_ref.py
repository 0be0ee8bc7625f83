"""The DTW score in double precision, and what early abandon claims about it, in plain numpy: the reference every DTW kernel's detect-only
path is held to (tests/test_gpu_abandon_edges.py) and the f64 evaluation tests/test_gpu_dtw_f64.py measures the arithmetics against.

Restated from the reference -- window cut + mean normalisation (wakeword_comp.rs:22-27, normalizer.rs:3-31), cosine distance
(comparator.rs:15-48), banded DTW read at D[m-1][n] (dtw.rs:56-105), cost / (m + n) -> logistic (comparator.rs:18-26) -- and pinned on the
CPU by tests/test_abandon_ref.py: against the strict-f32 oracle, and the theorem early abandon rests on.

Early abandon (detect-only calls in ScoreMode::Max): cell costs are >= 0 and every warping path from D[0][0] to the read-out cell D[m-1][n]
crosses every row 1..m-1 and every column 1..n inside the band, so the cheapest band cell of such a row or column is a lower bound of
D[m-1][n].  Once it exceeds nc_max(threshold, score_ref) * (m + n) the score cannot exceed `threshold` any more.  Row m is NOT such a row
(the read-out cell lies in row m-1): test_abandon_ref.py keeps an example.
"""
import numpy as np

from scan_ref import scan_ref


def f64_dtw(mfcc, tpl, band, n_win=None):
    """-> D [windows][m+1][n+1] in double precision (cells outside the band +inf), every window of every stream at once.

    mfcc: [n_frames][K] or [S][n_frames][K] f32 frames; tpl: [m][K] f32 template.  Window w of a stream is its frames w .. w + m - 1 (the
    reference cuts the window to the template's length); n_win: windows per stream (default: all that fit).  Rows = template frames
    (first sequence), columns = window frames; row r meets columns max(1, r - w) .. min(n, r + w - 1) (dtw.rs:56-105)."""
    x = np.asarray(mfcc, np.float64)
    if x.ndim == 2:
        x = x[None]
    a = np.asarray(tpl, np.float64)
    m = n = a.shape[0]
    if n_win is None:
        n_win = x.shape[1] - m + 1
    idx = np.arange(n_win)[:, None] + np.arange(n)[None, :]
    win = x[:, idx].reshape(x.shape[0] * n_win, n, x.shape[2])     # [S * n_win][n][K]
    win = win - win.sum(axis=1, keepdims=True) / n                  # MfccNormalizer::normalize of the cut window
    na = (a * a).sum(axis=1)                                        # [m]
    nb = (win * win).sum(axis=2)                                    # [windows][n]
    w = max(band, 0)
    D = np.full((win.shape[0], m + 1, n + 1), np.inf)
    D[:, 0, 0] = 0.0
    for r in range(1, m + 1):
        lo = max(1, r - w) if r > w else 1
        hi = min(n + 1, r + w)
        for c in range(lo, hi):
            mag = np.sqrt(na[r - 1] * nb[:, c - 1])
            dot = win[:, c - 1, :] @ a[r - 1]
            cos = np.where(mag == 0.0, 0.0, dot / np.where(mag == 0.0, 1.0, mag))
            D[:, r, c] = (1.0 - cos) + np.minimum(np.minimum(D[:, r - 1, c], D[:, r, c - 1]), D[:, r - 1, c - 1])
    return D


def logistic(nc, score_ref):
    """comparator.rs:18-26"""
    return 1.0 / (1.0 + np.exp((nc - score_ref) / score_ref))


def f64_nc_scores(mfcc, templates, band, score_ref, n_win=None):
    """-> (nc, score), each [windows][T] in double precision: nc = D[m-1][n] / (m + n) and its logistic.  Templates may differ in length;
    n_win (per stream) defaults to the windows the longest template fits in."""
    x = np.asarray(mfcc)
    nf = x.shape[-2]
    if n_win is None:
        n_win = nf - max(len(t) for t in templates) + 1
    nc = []
    for tpl in templates:
        m = len(tpl)
        nc.append(f64_dtw(x, tpl, band, n_win)[:, m - 1, m] / (m + m))
    nc = np.stack(nc, axis=1)
    return nc, logistic(nc, score_ref)


def f64_scores(mfcc, templates, band=5, score_ref=0.22):
    """Score[w][t] in double precision from the f32 frames and f32 templates (the reference's inputs) of ONE stream, every window the
    templates (of one length) fit in."""
    return f64_nc_scores(mfcc, templates, band, score_ref)[1]


def nc_max(threshold, score_ref):
    """The exact bound: score(nc) > threshold <=> nc < score_ref * (1 + ln(1 / threshold - 1)), threshold in (0, 1).  (The kernels' own
    bound, dtw_abandon_nc in rp_dtw.hip, is this one times 1.001 plus 1e-4: room for the rounding of the f32 running costs.)"""
    return score_ref * (1.0 + np.log(1.0 / threshold - 1.0))


def kernel_abandon_nc(threshold, score_ref):
    """dtw_abandon_nc (rp_dtw.hip) as it is written, in f32, for 0 < threshold < 1"""
    f = np.float32
    nc = f(score_ref) * (f(1) + np.log(f(1) / f(threshold) - f(1), dtype=np.float32))
    return f(nc * f(1.001) + f(1e-4)) if nc > 0 else f(nc + f(1e-4))


def reference_detections(agg, n_frames, max_len, threshold, min_scores, avg=None, avg_threshold=0.0, eager=False):
    """tests/scan_ref.py over the f64 Max aggregates: agg [S][n_win] (avg likewise, or None: no averaged-template test; with it the gate is
    applied as the reference does, wakeword_comp.rs:85-93) -> per stream [(frame, window, counter, avg_score, score)]."""
    agg = np.asarray(agg)
    return [scan_ref(agg[s], None if avg is None else np.asarray(avg)[s], n_frames, max_len, threshold, avg_threshold, min_scores, eager, None, 0.0)
            for s in range(agg.shape[0])]
