"""Early abandon of every DTW kernel's detect-only path, held to f64 (tests/abandon_ref.py).

A detect-only call in ScoreMode::Max (rp_batch_detect without `scores` / `agg`) may stop a wave whose every (window, template) is past
dtw_abandon_nc(threshold, score_ref) * (m + n) and write score 0 for them.  Here the per-window score workspace of such a call is read back
(rp_ctx_last_window_scores) and every DTW is compared with the kernel's own full call (bit-equal, or exactly 0) and with the f64 score of the
thing an abandoned DTW claims ("below the threshold") -- at the lengths where each kernel's check starts, has only its tail check, or has no
tail; in tiles and waves whose last lanes are invalid; with digital silence in a stream; at thresholds chosen from the f64 aggregates.

Where the checks are (derived from the kernels):
  dtw_mfma_kernel, eight slots / dtw_mfma_wide_kernel: the first 12 columns are one guarded block, a check before every further block of 12
      and one before the tail columns -> a template is checked when L > 12.
  dtw_mfma_kernel, four slots / dtw_mfma_wide3_kernel / dtw_ragged_kernel: blocks of 16 -> L > 16.
  dtw_band_kernel / dtw_band2_kernel / dtw_band_wide_kernel: the first 2W rows are guarded, a check before every further 2W rows -> L > 1 + 2W.
The ABI names kernel FAMILIES, the product arithmetic and the wave build (rp_ctx_dtw_kernels); which instantiation of a family a template set
takes follows from its chunk classes (launch_dtw_k5 / launch_dtw_wide_all, rp_dtw.hip) and is named in the case tables below.

Two cases stand apart from the table: a window that is alive only through the edge cell of its band (the minimum runs over every cell), and
one live stream, where the averaged template is scored under the bound and only the kernels' guards keep it.

RP_ABANDON_EDGES_PROFILE=<file>: the share of DTWs abandoned per case and threshold is written there (profiles/abandon_edges.txt).
"""
import os
import time

import numpy as np
import pytest

import abandon_ref as ar
from oracle import rp_oracle as orc

SEED = 0x5EED000000000001
SCORE_REF = 0.22
QUANTILES = (("q50", 0.5), ("q90", 0.9), ("q99", 0.99))
MFMA, WIDE, RAGGED, REG = "dtw_mfma_kernel", "dtw_mfma_wide_kernel", "dtw_ragged_kernel", "register kernels"

SHARES = []          # (case name, route, threshold name, threshold, share abandoned)
_T0 = []            # when the first case was built
_CASES = {}


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


class env:
    """launch switches that are read per call (RP_DTW_NO_FUSED_MAX, RP_DTW_NO_SPLIT) for the calls inside"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ one case: streams, templates, the f64 reference, thresholds
class Case:
    pass


def build_case(ctx, K, lens, band, S=5, n_win_min=100, silence=True, silent_tail=0):
    """S streams of about n_win_min windows (S x n_win never a multiple of 64: the last matrix tile and the last vector wave have invalid
    lanes), stream 1 with a stretch of digital silence, the kernel's own MFCC frames scored in f64.  Shared by every test of the shape."""
    key = (K, tuple(lens), band, S, n_win_min, silence, silent_tail)
    if key in _CASES:
        return _CASES[key]
    if not _T0:
        _T0.append(time.time())
    c = Case()
    c.K, c.lens, c.band, c.S, c.T, c.L = K, list(lens), band, S, len(lens), max(lens)
    chunks = (n_win_min + c.L - 1 + 3 + 2) // 3
    c.nf = 3 * chunks - 3
    c.n_win = c.nf - c.L + 1
    assert c.n_win >= n_win_min and (S * c.n_win) % 64 != 0
    seed_t = SEED + 31 * K + 7 * c.L + band
    c.templates = [t[:n].copy() for t, n in zip(orc.synth_templates(seed_t, c.T, c.L, K), lens)]
    c.pcm = ctx.synth_pcm(SEED, 40 + c.L, S, 480 * chunks)
    # the utterances the first templates were made of (orc.synth_templates: seeds seed + 1 + t, stream 0), one in each of streams 2, 3, 4: a
    # handful of windows score near the top of the logistic, so the 0.99-quantile threshold lies among them and the bound it sets
    # (nc_max ~ 0.05) is one most windows pass early -- and the detections of (6) are real ones
    n_utt = 480 * ((c.L + 3 + 2) // 3)
    for i in range(3):
        c.pcm[2 + i, 480 * (1 + i):480 * (1 + i) + n_utt] = orc.synth_pcm(seed_t + 1 + i % c.T, 0, n_utt)
    if silence:   # stream 1 from its eighth chunk on: the windows inside are zero vectors after the mean is taken out (similarity 0, the
        # lowest score there is) -- whole matrix tiles and whole vector waves of them, next to waves that straddle speech and silence
        c.pcm[1, 480 * 7:] = 0.0
    if silent_tail:   # the last streams are silence throughout and stream 0 begins with the first template's utterance: see assertion (7)
        c.pcm[S - silent_tail:] = 0.0
        c.pcm[0, :n_utt] = orc.synth_pcm(seed_t + 1, 0, n_utt)
    c.mf = ctx.mfcc(c.pcm, K)
    assert c.mf.shape == (S, c.nf, K)
    nc, sc = ar.f64_nc_scores(c.mf, c.templates, band, SCORE_REF, c.n_win)
    c.nc64, c.sc64 = nc.reshape(S, c.n_win, c.T), sc.reshape(S, c.n_win, c.T)
    c.agg64 = c.sc64.max(axis=2)
    c.thresholds = [("t999", 0.999)] + [(name, gap_threshold(c.agg64, q)) for name, q in QUANTILES]
    # Just inside the bound: a window of silence costs exactly 1 per cell, D[m-1][n] = L, nc = 0.5 in every arithmetic.  With the threshold a
    # thousandth below that score, whole tiles and waves of such windows can still fire and sit 0.06 % inside the exact bound all the way:
    # their last checks see 92 % and more of the final cost (lengths 13, 17, 25, 33, 2Wk + 2), so a bound a tenth too tight, or one taken
    # of m instead of m + n, drops them
    silent = np.abs(c.nc64 - 0.5).max(axis=2) < 1e-12
    s_sil = float(ar.logistic(0.5, SCORE_REF))
    thr = float(np.float32(s_sil * (1.0 - 1e-3)))
    # (a condition on the input, as in gap_threshold: no other aggregate within the parity gate of this threshold -- a window that is
    # silent only in part can score just below silence where templates are short; such a case goes without this threshold)
    if silent.sum() >= 64 and not ((c.agg64 > thr * (1.0 - 1e-4)) & (c.agg64 < s_sil * (1.0 - 1e-9))).any():
        c.thresholds.append(("tsil", thr))
    # (7) the rows from the last multiple of 128 on are the final, partial tile or wave of every kernel (32, 64 or 128 rows each)
    c.tail_row = (S * c.n_win) // 128 * 128 if silent_tail else None
    if silent_tail:
        assert silent.reshape(-1)[c.tail_row:].all() and c.tail_row < S * c.n_win
    _CASES[key] = c
    return c


def gap_threshold(values, q):
    """the midpoint of the widest gap among the 16 sorted values around the q-quantile; the gap is at least 4e-5 of it (the 1e-5 parity gate
    on both sides, doubled) -- a condition on the input: a seed that does not meet it is changed, not the factor"""
    v = np.sort(np.asarray(values, np.float64).ravel())
    i = int(round(q * (v.size - 1)))
    lo = min(max(0, i - 8), v.size - 16)
    seg = v[lo:lo + 16]
    j = int(np.argmax(np.diff(seg)))
    thr = 0.5 * (seg[j] + seg[j + 1])
    assert seg[j + 1] - seg[j] >= 4e-5 * thr, (q, seg[j], seg[j + 1])
    return float(np.float32(thr)) if seg[j] < float(np.float32(thr)) < seg[j + 1] else thr


def check_points(route, L, band):
    """the rows (register kernels) or columns (matrix kernels) a DTW of L frames has behind it at each of its abandon checks (see the head
    of the file): after every 2W rows while rows are left (r0 = 1 + rows < L); after every block of 12 / 16 columns while columns are left"""
    if route == "reg":
        return [r for r in range(2 * band, L, 2 * band) if 1 + r < L]
    return list(range({"mfma8": 12, "wide": 12, "mfma4": 16, "wide3": 16, "ragged": 16}[route], L, {"mfma8": 12, "wide": 12}.get(route, 16)))


def checked(route, L, band):
    """does a template of L frames meet an abandon check at all: L > 12 / L > 16 / L > 1 + 2W"""
    return bool(check_points(route, L, band))


def _config(ra, case, thr, min_scores=1):
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold, cfg.min_scores = 0.0, thr, min_scores
    cfg.band_size, cfg.score_ref = case.band, SCORE_REF
    return cfg


def _same_detections_as_f64(case, det, n_det, want, max_det):
    for s in range(case.S):
        assert n_det[s] == len(want[s]), (s, n_det[s], want[s])
        for d, w in zip(det[s][:min(n_det[s], max_det)], want[s]):
            assert (d["frame"], d["window"], d["counter"]) == w[:3], (s, d, w)
            assert abs(float(d["score"]) - float(w[4])) <= 1e-5 * float(w[4]), (s, d, w)


def check_case(ra, ctx, tm, case, name, route, expect, thr_name, thr, max_det=8, record=True):
    """assertions (1) route, (2) bit-equal or 0, (3) sound against f64, (4) cadence at 0.999, (5) effect at q99, (6) detections and (7) a
    final wave of silence of one (case, threshold); -> the detect-only call's workspace"""
    kernels, products, waves = expect
    cfg = _config(ra, case, thr)
    pairs = ctx.dtw_ref_pairs()
    d_full, n_full, sc_full, agg_full = ctx.batch_detect(case.pcm, tm, cfg, max_det=max_det, want_scores=True)
    ctx.dtw_kernels()
    d_fast, n_fast = ctx.batch_detect(case.pcm, tm, cfg, max_det=max_det)
    ran = ctx.dtw_kernels()
    ws = ctx.last_window_scores(case.S, case.n_win, case.T)
    where = (name, thr_name, thr)
    # the premise that no fix-listed window is among the abandoned ones: frames made from finite PCM stay inside the norm range (log-mel
    # coefficients; silence centres to exact zeros), so nothing is ever listed for dtw_ref_kernel -- the abandon-then-list path of the
    # kernels is not reached through rp_batch_detect
    assert ctx.dtw_ref_pairs() == pairs, where
    # (1) the route: a case that silently runs another kernel is a failure, not a pass
    assert set(ran) == set(kernels) and ctx.last_dtw_products == products and ctx.last_dtw_mfma_waves == waves, \
        (where, ran, ctx.last_dtw_products, ctx.last_dtw_mfma_waves)
    # (2) per DTW against the kernel's own full call: the same bits, or exactly 0
    assert sc_full.shape == ws.shape == case.sc64.shape and (sc_full > 0).all()
    zero = _bits(ws) == 0
    same = _bits(ws) == _bits(sc_full)
    assert (zero | same).all(), (where, int((~(zero | same)).sum()), np.argwhere(~(zero | same))[:4])
    # (3) soundness against f64, no tolerance: an abandoned DTW's score is below the threshold
    bad = zero & ~(case.sc64 < thr)
    assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4], case.sc64[bad][:4])
    share = float(zero.mean())
    per_len = {L: float(zero[:, :, [t for t in range(case.T) if case.lens[t] == L]].mean()) for L in sorted(set(case.lens))}
    if record:
        SHARES.append((name, route, thr_name, thr, share))
    print("%-44s %-7s %s %.6f abandoned %.4f %s" % (name, route, thr_name, thr, share, per_len if len(per_len) > 1 else ""))
    # (4) cadence: at 0.999 the bound is negative, every DTW that meets a check dies at its first one -- in partial tiles and waves too --
    #     and a DTW that meets none keeps the full call's bits
    if thr_name == "t999":
        for t in range(case.T):
            if checked(route, case.lens[t], case.band):
                assert zero[:, :, t].all(), (where, t, case.lens[t], float(zero[:, :, t].mean()))
            else:
                assert same[:, :, t].all() and not zero[:, :, t].any(), (where, t, case.lens[t])
    # (5) effect: (2) and (3) do not pass vacuously
    if thr_name == "q99" and any(checked(route, L, case.band) for L in case.lens):
        assert share > 0, where
    # (7) a final partial tile or wave of silence only: a silent DTW has cost exactly k after k rows or columns, so it is past the kernels'
    #     own bound at a check by a margin we can name -- then the wave must stop, whatever its invalid lanes hold (they must not vote)
    if case.tail_row is not None and thr_name in ("q90", "q99"):
        for t in range(case.T):
            L = case.lens[t]
            if any(k > 1.01 * float(ar.kernel_abandon_nc(thr, SCORE_REF)) * 2 * L for k in check_points(route, L, case.band)):
                assert zero.reshape(-1, case.T)[case.tail_row:, t].all(), (where, t, "a wave of silence with invalid lanes was not abandoned")
    # (6) detections: the full call's bytes, and the f64 aggregates' through the reference's state machine
    assert np.array_equal(n_fast, n_full) and d_fast.tobytes() == d_full.tobytes(), where
    want = ar.reference_detections(case.agg64, case.nf, case.L, thr, cfg.min_scores)
    _same_detections_as_f64(case, d_full, n_full, want, max_det)
    return ws


def run_case(ra, ctx, name, route, expect, K, lens, band, record=True, **kw):
    case = build_case(ctx, K, lens, band, **kw)
    tm = ra.Templates(ctx, case.templates)
    out = {}
    for thr_name, thr in case.thresholds:
        out[thr_name] = check_case(ra, ctx, tm, case, name, route, expect, thr_name, thr, record=record)
    return case, out


# expected (families, products, wave builds) of the detect-only call
X_MFMA8 = ([MFMA], ["bf16x3"], [8])      # dtw_mfma_kernel<W, 8, false, 8, true>: early abandon keeps the eight-wave build
X_MFMA4 = ([MFMA], ["bf16x3"], [12])     # dtw_mfma_abandon_kernel<5, 12, false, 4, true>
X_WIDE3 = ([WIDE], ["bf16x3"], [])
X_REG = ([REG], [], [])
X_SPLIT8 = ([MFMA], ["f16x2"], [12])     # the two-part dtw_mfma_kernel<W, 12, false, 8, false>, check compiled in
X_SPLITW = ([WIDE], ["f16x2"], [])       # dtw_mfma_wide_kernel


# ------------------------------------------------------------------ the case table, f32_matrix
@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused_max", "no_fused_max"])
@pytest.mark.parametrize("L", [12, 13, 25, 36])
@pytest.mark.parametrize("band", [3, 4, 5])
def test_eight_slot_matrix_kernel(ra, ctx, band, L, fused):
    """dtw_mfma_kernel, eight template slots, eight waves: one guarded block alone (12: never checked), the tail check alone (13), a block
    check and the tail check (25), three blocks and no tail (36); ScoreMode::Max inside the kernel and by the aggregate pass."""
    with env(**({} if fused else {"RP_DTW_NO_FUSED_MAX": "1"})):
        run_case(ra, ctx, "f32_matrix K5 T8 L%d band%d%s" % (L, band, "" if fused else " no-fuse"), "mfma8", X_MFMA8, 5, [L] * 8, band)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [16, 17, 33, 48])
@pytest.mark.parametrize("T", [4, 3])
def test_four_slot_matrix_kernel(ra, ctx, T, L):
    """chunks of 3..4 templates at band 5: dtw_mfma_abandon_kernel<5, 12, false, 4, true>, blocks of 16 columns"""
    run_case(ra, ctx, "f32_matrix K5 T%d L%d band5" % (T, L), "mfma4", X_MFMA4, 5, [L] * T, 5)


@pytest.mark.gpu
def test_two_chunks_of_the_eight_slot_kernel(ra, ctx):
    """13 templates of one length = chunks of 8 + 5: no fused Max, the second chunk with three empty slots"""
    run_case(ra, ctx, "f32_matrix K5 T13 L25 band5", "mfma8", X_MFMA8, 5, [25] * 13, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("no_split", [True, False], ids=["tc8", "tc4_half_chunks"])
@pytest.mark.parametrize("L", [13, 14, 30])
def test_band6_eight_templates_register_kernel(ra, ctx, L, no_split):
    """band 6 has no matrix kernel: dtw_band_kernel<5, 6, 8> (RP_DTW_NO_SPLIT=1) or its <5, 6, 4> half chunks (a batch this small)"""
    with env(**({"RP_DTW_NO_SPLIT": "1"} if no_split else {})):
        run_case(ra, ctx, "f32_matrix K5 T8 L%d band6 %s" % (L, "tc8" if no_split else "tc4"), "reg", X_REG, 5, [L] * 8, 6)


LATE = {3: 26, 4: 26, 5: 32, 6: 26}   # 2Wk + 2: the last check comes two rows before the end


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["2W+1", "2W+2", "30", "late"])
@pytest.mark.parametrize("band", [3, 4, 5, 6])
@pytest.mark.parametrize("T", [2, 1])
def test_pairs_and_single_templates_register_kernels(ra, ctx, T, band, which):
    """two templates: dtw_band_kernel<5, W, 2>; one: dtw_band2_kernel<5, W> (two windows per lane, waves of 128 entries)"""
    L = (2 * band + 1, 2 * band + 2, 30, LATE[band])[which]
    run_case(ra, ctx, "f32_matrix K5 T%d L%d band%d" % (T, L, band), "reg", X_REG, 5, [L] * T, band)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [16, 17, 33])
@pytest.mark.parametrize("K", [13, 16])
def test_wide_three_part_matrix_kernel(ra, ctx, K, L):
    """mfcc_size 13 / 16, three templates of one length, band 5: dtw_mfma_wide3_kernel (reported as dtw_mfma_wide_kernel + bf16x3)"""
    run_case(ra, ctx, "f32_matrix K%d T3 L%d band5" % (K, L), "wide3", X_WIDE3, K, [L] * 3, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1], ids=["2W+2", "30"])
@pytest.mark.parametrize("band", [3, 4, 5, 6])
@pytest.mark.parametrize("T", [2, 1])
@pytest.mark.parametrize("K", [13, 16])
def test_wide_register_kernel(ra, ctx, K, T, band, which):
    """mfcc_size 13 / 16, one or two templates: dtw_band_wide_kernel<K, W, 1 / 2>"""
    L = (2 * band + 2, 30)[which]
    run_case(ra, ctx, "f32_matrix K%d T%d L%d band%d" % (K, T, L, band), "reg", X_REG, K, [L] * T, band)


# ------------------------------------------------------------------ the other arithmetics
@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["2W+1", "2W+2", "30", "late"])
@pytest.mark.parametrize("band", [3, 4, 5, 6])
@pytest.mark.parametrize("T", [4, 8])
def test_strict_f32_register_kernels(ra, ctx, T, band, which):
    """strict_f32: dtw_band_kernel<5, W, 4> and <5, W, 8> (RP_DTW_NO_SPLIT=1: a batch this small would take the half chunks) score what the
    matrix kernels score by default"""
    L = (2 * band + 1, 2 * band + 2, 30, LATE[band])[which]
    with ctx.arithmetic("strict_f32"), env(RP_DTW_NO_SPLIT="1"):
        run_case(ra, ctx, "strict_f32 K5 T%d L%d band%d" % (T, L, band), "reg", X_REG, 5, [L] * T, band)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [13, 25])
@pytest.mark.parametrize("band", [3, 5])
def test_fast_split_eight_slot_matrix_kernel(ra, ctx, band, L):
    """fast_split: the two-part dtw_mfma_kernel, twelve waves, the check compiled into the kernel itself"""
    with ctx.arithmetic("fast_split"):
        run_case(ra, ctx, "fast_split K5 T8 L%d band%d" % (L, band), "mfma8", X_SPLIT8, 5, [L] * 8, band)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [17, 33])
def test_fast_split_wide_matrix_kernel(ra, ctx, L):
    """fast_split, mfcc_size 16, eight templates: dtw_mfma_wide_kernel (blocks of 12 columns)"""
    with ctx.arithmetic("fast_split"):
        run_case(ra, ctx, "fast_split K16 T8 L%d band5" % L, "wide", X_SPLITW, 16, [L] * 8, 5)


@pytest.mark.gpu
def test_fast_split_ragged_matrix_kernel(ra, ctx):
    """fast_split + ragged_matrix, five lengths: dtw_ragged_kernel; the windows it cannot resolve (the silence) go to the register kernels'
    list mode, which is handed the same bound"""
    with ctx.arithmetic("fast_split", ragged_matrix=True):
        run_case(ra, ctx, "fast_split+ragged K5 L20..40 band5", "ragged", ([RAGGED, REG], ["f16x2"], []), 5, [20, 26, 31, 37, 40], 5)


# ------------------------------------------------------------------ few windows per stream: frames from global memory (the GX builds)
@pytest.mark.gpu
@pytest.mark.parametrize("name,route,expect,K,lens,band", [
    ("GX f32_matrix K5 T8 L25 band5", "mfma8", X_MFMA8, 5, [25] * 8, 5),
    ("GX f32_matrix K5 T8 L13 band3", "mfma8", X_MFMA8, 5, [13] * 8, 3),
    ("GX f32_matrix K5 T4 L33 band5", "mfma4", X_MFMA4, 5, [33] * 4, 5),
    ("GX f32_matrix K5 T3 L17 band5", "mfma4", X_MFMA4, 5, [17] * 3, 5),
    ("GX f32_matrix K16 T3 L33 band5", "wide3", X_WIDE3, 16, [33] * 3, 5),
    ("GX f32_matrix K13 T3 L17 band5", "wide3", X_WIDE3, 13, [17] * 3, 5),
    ("GX f32_matrix K5 T2 L12 band5", "reg", X_REG, 5, [12] * 2, 5),
    ("GX f32_matrix K5 T1 L30 band4", "reg", X_REG, 5, [30], 4),
    ("GX f32_matrix K5 T8 L14 band6", "reg", X_REG, 5, [14] * 8, 6),
    ("GX f32_matrix K16 T2 L30 band5", "reg", X_REG, 16, [30] * 2, 5),
], ids=["mfma8_L25", "mfma8_L13_band3", "mfma4_L33", "mfma4_L17", "wide3_K16", "wide3_K13", "band_pair_L12", "band2_L30", "band6_T8", "band_wide_K16"])
def test_few_windows_per_stream(ra, ctx, name, route, expect, K, lens, band):
    """40 streams with fewer than 64 windows each: cross-stream waves that read their frames from global memory.  Still rp_batch_detect:
    the workspace is defined and assertions (1) to (6) apply.  The last seven streams are silence: the final partial tile or wave holds
    nothing else (7)."""
    case, _ = run_case(ra, ctx, name, route, expect, K, lens, band, S=40, n_win_min=13, silence=True, silent_tail=7)
    assert case.n_win < 64 and (case.S * case.n_win) % 64 != 0
    # (7) is armed: the first window of the call -- what a lane past the end may be pointed at -- is above the q90 threshold, the tail is not,
    # and the tail's DTWs meet a check past the bound at q99
    thr = dict(case.thresholds)
    assert case.agg64[0, 0] > thr["q90"] and case.tail_row is not None
    assert any(k > 1.01 * float(ar.kernel_abandon_nc(thr["q99"], SCORE_REF)) * 2 * case.L for k in check_points(route, case.L, case.band))


# ------------------------------------------------------------------ live-stream batches: detections only
@pytest.mark.gpu
@pytest.mark.parametrize("arith,ragged,K,lens,band", [
    ("f32_matrix", False, 5, [25] * 8, 5), ("f32_matrix", False, 5, [33] * 4, 5), ("f32_matrix", False, 16, [33] * 3, 5),
    ("f32_matrix", False, 5, [30] * 2, 4), ("f32_matrix", False, 5, [30], 6), ("f32_matrix", False, 13, [30] * 2, 5),
    ("strict_f32", False, 5, [30] * 8, 5), ("fast_split", False, 5, [25] * 8, 3), ("fast_split", False, 16, [33] * 8, 5)],
    ids=["mfma8", "mfma4", "wide3", "band_pair", "band2", "band_wide", "strict_f32", "split_mfma8", "split_wide"])
def test_live_stream_batches_report_the_offline_detections(ra, ctx, arith, ragged, K, lens, band):
    """The same streams fed to a StreamBatch 1 and 3 chunks per call (no per-window aggregates asked: early abandon on): the detections of the
    offline full call, field by field.  (No row for dtw_ragged_kernel: it needs 64 windows per stream, a live batch never launches it.)"""
    with ctx.arithmetic(arith, ragged_matrix=ragged):
        case = build_case(ctx, K, lens, band)
        tm = ra.Templates(ctx, case.templates)
        fired = 0
        for thr_name, thr in case.thresholds[2:]:     # q90, q99
            cfg = _config(ra, case, thr)
            d_full, n_full, _, _ = ctx.batch_detect(case.pcm, tm, cfg, max_det=8, want_scores=True)
            fired += int(n_full.sum())
            for k in (1, 3):
                sb = ra.StreamBatch(ctx, tm, cfg, case.S, max_chunks_per_call=k)
                live = [[] for _ in range(case.S)]
                for i in range(0, case.pcm.shape[1], 480 * k):
                    d, nd = sb.process(np.ascontiguousarray(case.pcm[:, i:i + 480 * k]), max_det=8)
                    for s in range(case.S):
                        live[s] += [d[s][j] for j in range(nd[s])]
                for s in range(case.S):
                    assert len(live[s]) == n_full[s], (thr_name, k, s)
                    for a, b in zip(live[s], d_full[s][:n_full[s]]):
                        assert (a["frame"], a["window"], a["counter"], a["score"]) == (b["frame"], b["window"], b["counter"], b["score"]), (thr_name, k, s)
        assert fired > 0, "the case must produce detections"


# ------------------------------------------------------------------ the averaged-template gate together with early abandon
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["list", "dense"])
@pytest.mark.parametrize("arith,K,T,L,band", [("f32_matrix", 5, 8, 25, 5), ("f32_matrix", 5, 2, 30, 4), ("strict_f32", 5, 8, 30, 5), ("f32_matrix", 16, 3, 33, 5)],
                         ids=["mfma8", "band_pair", "strict_f32", "wide3"])
def test_gate_with_early_abandon(ra, arith, K, T, L, band, mode):
    """gated_register hands abandon_nc to its list-mode and dense-mode launches.  avg_threshold at the median f64 averaged-template score (a
    sparse list) and low enough that more than 90 % of the rows pass (dense_min: the staged launch over every window): the detections of the
    context that scores everything, and of the f64 scores with the gate applied; the averaged template is never abandoned."""
    gated, full = ra.BatchContext(0, arithmetic=arith), ra.BatchContext(0, full_scores=True, arithmetic=arith)
    case = build_case(gated, K, [L] * T, band, silence=False)   # (fully silent windows tie at the bottom of the averaged-template scores)
    avg_t = np.mean(case.templates, axis=0, dtype=np.float32)
    avg64 = ar.f64_nc_scores(case.mf, [avg_t], band, SCORE_REF, case.n_win)[1].reshape(case.S, case.n_win)
    avg_thr = gap_threshold(avg64, 0.5 if mode == "list" else 0.03)
    # which launch of gated_register scores the rows is decided on the device: the list when fewer than dense_min = rows - rows / 10 rows
    # pass (rp_dtw.hip), else the staged launch over every window.  Nothing observable names it, so the premise is stated here: a change of
    # dense_min has to move these two thresholds with it
    rows = case.S * case.n_win
    dense_min, listed = rows - rows // 10, int((avg64 >= avg_thr).sum())
    assert (0.3 * rows < listed < 0.7 * rows) if mode == "list" else listed >= dense_min + rows // 50
    tg, tf = ra.Templates(gated, case.templates, avg=avg_t), ra.Templates(full, case.templates, avg=avg_t)
    fired = 0
    for thr_name, thr in case.thresholds:
        cfg = _config(ra, case, thr)
        cfg.avg_threshold = avg_thr
        d_g, n_g = gated.batch_detect(case.pcm, tg, cfg, max_det=8)
        d_f, n_f = full.batch_detect(case.pcm, tf, cfg, max_det=8)
        assert np.array_equal(n_g, n_f) and d_g.tobytes() == d_f.tobytes(), (thr_name, thr)
        want = ar.reference_detections(case.agg64, case.nf, case.L, thr, cfg.min_scores, avg=avg64, avg_threshold=avg_thr)
        _same_detections_as_f64(case, d_g, n_g, want, 8)
        for s in range(case.S):
            for d, w in zip(d_g[s][:n_g[s]], want[s]):
                assert d["avg_score"] > 0 and abs(float(d["avg_score"]) - float(w[3])) <= 1e-5 * float(w[3]), (thr_name, s, d, w)
        fired += int(n_g.sum())
        if thr_name == "t999":
            assert n_g.sum() == 0
    assert fired > 0, "the case must produce detections"


# ------------------------------------------------------------------ the band-edge cell: the minimum is taken over EVERY band cell
def build_edge_case(ctx, kind, T, band=5, S=5):
    """One window whose cheapest warping path runs along the edge cell of the band (q = 0 of the kernels' running costs) at cost 0, every
    other cell of the band a speech frame's distance away, scored against a template cut from the stream's own centred frames.
    kind "rows" (the register kernels check rows: q = 0 is column r - W): the first window of stream 0, silence behind its speech; template
    rows 1..W+1 are column 1, row r is column r - W, and row m-1 meets the silence, which carries it to column n for nothing.
    kind "cols" (the matrix kernels check columns: q = 0 is row c - W + 1): the last window of stream 2, W + 1 frames of silence at its head;
    row 1 meets them all, row r is column r + W - 1, the last W rows are column n.
    With the threshold a thousandth below that window's score the bound is 0.06 cost units: a minimum that skips q = 0 abandons it."""
    key = ("edge", kind, T, band, S)
    if key in _CASES:
        return _CASES[key]
    if not _T0:
        _T0.append(time.time())
    K, W, chunks = 5, band, 40
    c = Case()
    c.K, c.band, c.S, c.T, c.nf = K, band, S, T, 3 * chunks - 3
    c.pcm = ctx.synth_pcm(SEED, 300, S, 480 * chunks)
    if kind == "rows":
        c.s0 = 0
        c.pcm[0, 160 * 26:] = 0.0
        mf = ctx.mfcc(c.pcm, K)
        sil = (mf[0] == mf[0, -1]).all(axis=1)
        b = int(c.nf - np.argmin(sil[::-1]))            # the first frame of the silence
        # (neighbouring speech frames are close -- they share two thirds of their samples -- so the check that counts is the one at row
        # 2Wk = b + W, where the edge cell is the last speech column and its neighbour the first of the silence: L = 32, row 30)
        assert b == 25 and sil[b:].all() and not sil[:b].any()
        c.L = b + W + 2
        start, c.w0 = 0, 0
        cols = [max(1, r - W) for r in range(1, c.L + 1)]
    else:
        c.s0 = 2
        c.pcm[2, 160 * 82:160 * 93] = 0.0
        mf = ctx.mfcc(c.pcm, K)
        sil = (mf[2] == mf[2, 86]).all(axis=1)
        q = int(np.flatnonzero(sil).max()) + 1           # the first frame of speech behind the silence
        assert sil[q - W - 1:q].all() and not sil[q:].any() and 84 <= q - W - 1 <= 92
        start = q - W - 1
        c.L = c.nf - start
        cols = [min(c.L, r + W - 1) for r in range(1, c.L + 1)]
    c.n_win = c.nf - c.L + 1
    if kind == "cols":
        c.w0 = c.n_win - 1
    c.lens = [c.L] * T
    win = mf[c.s0, start:start + c.L].astype(np.float64)
    y = win - win.sum(axis=0) / c.L
    special = np.stack([y[col - 1] for col in cols]).astype(np.float32)
    c.templates = [special] + list(orc.synth_templates(SEED + 900 + c.L, T - 1, c.L, K)) if T > 1 else [special]
    c.mf = mf
    nc, sc = ar.f64_nc_scores(mf, c.templates, band, SCORE_REF, c.n_win)
    c.nc64, c.sc64 = nc.reshape(S, c.n_win, T), sc.reshape(S, c.n_win, T)
    c.agg64 = c.sc64.max(axis=2)
    top = c.sc64[c.s0, c.w0, 0]
    assert top == c.agg64[c.s0, c.w0] and top > 0.7310 and c.nc64[c.s0, c.w0, 0] < 1e-6     # the path of cost 0
    thr = float(np.float32(top * (1.0 - 1e-3)))
    others = c.agg64.copy()
    others[c.s0, c.w0] = 0.0
    assert others.max() < thr * (1.0 - 1e-4)            # a condition on the input, as in gap_threshold
    c.thresholds = [("tedge", thr)]
    c.tail_row = None
    c.D = ar.f64_dtw(mf[c.s0], special, band, c.n_win)[c.w0]
    _CASES[key] = c
    return c


def _edge_is_armed(case, kind, route, thr):
    """at one of the kernel's checks the edge cell is far inside the kernels' own bound and every other cell of the band far outside"""
    W, L, D = case.band, case.L, case.D
    bound = float(ar.kernel_abandon_nc(thr, SCORE_REF)) * 2 * L
    for k in check_points(route, L, W):
        if kind == "rows":
            edge, rest = D[k, k - W], D[k, k - W + 1:min(L, k + W - 1) + 1]
        else:
            edge, rest = D[k - W + 1, k], D[k - W + 2:min(L, k + W) + 1, k]
        if edge <= 0.01 * bound and rest.min() > 1.5 * bound:
            return True
    return False


@pytest.mark.gpu
@pytest.mark.parametrize("kind,T,route,expect", [("rows", 2, "reg", X_REG), ("rows", 1, "reg", X_REG), ("cols", 8, "mfma8", X_MFMA8), ("cols", 4, "mfma4", X_MFMA4)],
                         ids=["dtw_band_kernel", "dtw_band2_kernel", "dtw_mfma_kernel_8_slots", "dtw_mfma_kernel_4_slots"])
def test_the_band_edge_cell_counts(ra, ctx, kind, T, route, expect):
    """A DTW that is alive only through the edge cell of its band must not be abandoned: assertions (1) to (6) at a threshold just below its
    score -- (3) names it when a kernel takes the minimum over the other cells only, (6) misses its detection."""
    case = build_edge_case(ctx, kind, T)
    name, thr = case.thresholds[0]
    assert _edge_is_armed(case, kind, route, thr)
    tm = ra.Templates(ctx, case.templates)
    ws = check_case(ra, ctx, tm, case, "band edge %s K5 T%d L%d band5" % (kind, T, case.L), route, expect, name, thr)
    assert ws[case.s0, case.w0, 0] > thr and float((ws == 0).mean()) > 0.5     # it is kept, most of the others are not
    if kind == "rows":   # (the last window of a stream starts a detection that the end of the stream never reports)
        want = ar.reference_detections(case.agg64, case.nf, case.L, thr, 1)
        assert len(want[case.s0]) == 1 and want[case.s0][0][1] == case.w0


# ------------------------------------------------------------------ one live stream: the averaged template next to a finite bound
@pytest.mark.gpu
@pytest.mark.parametrize("K,T,family", [(5, 8, MFMA), (16, 3, WIDE)], ids=["dtw_band2_kernel", "dtw_band_wide_kernel"])
def test_one_live_stream_never_abandons_the_averaged_template(ra, K, T, family):
    """A live batch of ONE stream skips the gate (DtwScore::gate_one_stream) and scores the averaged template in the ungated launch, next
    to the sample templates and under the same finite bound: only the kernels' `tid < T` guards keep it from being abandoned there.  With a
    threshold among the planted utterances' scores the averaged template's DTWs are past the bound at their checks, and the detections must
    still carry its score: those of a context that scores everything, and of f64 with the gate applied."""
    L, band, chunks = 32, 5, 40
    live_ctx, full = ra.BatchContext(0), ra.BatchContext(0, full_scores=True)
    seed_t = SEED + 5000 + K
    templates = orc.synth_templates(seed_t, T, L, K)
    avg_t = np.mean(templates, axis=0, dtype=np.float32)
    n_utt = 480 * ((L + 3 + 2) // 3)
    pcm = live_ctx.synth_pcm(SEED, 77, 1, 480 * chunks)
    pcm[0, 480 * 5:480 * 5 + n_utt] = orc.synth_pcm(seed_t + 1, 0, n_utt)
    pcm[0, 480 * 23:480 * 23 + n_utt] = orc.synth_pcm(seed_t + 2, 0, n_utt)
    mf = live_ctx.mfcc(pcm, K)
    nf, n_win = mf.shape[1], mf.shape[1] - L + 1
    agg64 = ar.f64_nc_scores(mf, templates, band, SCORE_REF, n_win)[1].max(axis=1)[None]
    avg64 = ar.f64_nc_scores(mf, [avg_t], band, SCORE_REF, n_win)[1].reshape(1, n_win)
    thr = gap_threshold(agg64, 0.95)
    firing = np.flatnonzero(agg64[0] > thr)
    assert 2 <= firing.size <= 20
    avg_thr = float(np.float32(0.8 * avg64[0, firing].min()))
    assert (np.abs(avg64 - avg_thr) > 1e-4 * avg_thr).all()
    # armed: the averaged template's DTW of every window around the firing ones is past the kernels' bound at its last check (row 30)
    D = ar.f64_dtw(mf, avg_t, band, n_win)
    bound = float(ar.kernel_abandon_nc(thr, SCORE_REF)) * 2 * L
    near = np.unique(np.clip(firing[:, None] + np.arange(-3, 4)[None, :], 0, n_win - 1))
    assert (D[near, 30, 25:35].min(axis=1) > 1.05 * bound).all()
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold, cfg.min_scores, cfg.band_size, cfg.score_ref = avg_thr, thr, 1, band, SCORE_REF
    want = ar.reference_detections(agg64, nf, L, thr, 1, avg=avg64, avg_threshold=avg_thr)[0]
    assert len(want) >= 1
    d_f, n_f = full.batch_detect(pcm, ra.Templates(full, templates, avg=avg_t), cfg, max_det=8)
    sb = ra.StreamBatch(live_ctx, ra.Templates(live_ctx, templates, avg=avg_t), cfg, 1, max_chunks_per_call=1)
    live_ctx.dtw_kernels()
    live = []
    for i in range(0, pcm.shape[1], 480):
        d, nd = sb.process(np.ascontiguousarray(pcm[:, i:i + 480]), max_det=8)
        live += [d[0][j] for j in range(nd[0])]
    ran = live_ctx.dtw_kernels()
    assert family in ran and REG in ran and "dtw_single_kernel" not in ran, ran     # the batch kernels, the averaged template among them
    assert len(live) == n_f[0] == len(want), (len(live), n_f, want)
    for a, b, w in zip(live, d_f[0][:n_f[0]], want):
        assert (a["frame"], a["window"], a["counter"], a["score"], a["avg_score"]) == (b["frame"], b["window"], b["counter"], b["score"], b["avg_score"]), (a, b)
        assert (a["frame"], a["window"], a["counter"]) == w[:3], (a, w)
        assert abs(float(a["score"]) - float(w[4])) <= 1e-5 * float(w[4]) and abs(float(a["avg_score"]) - float(w[3])) <= 1e-5 * float(w[3]), (a, w)


# ------------------------------------------------------------------ RP_MFMA3_WAVES=12: read once per process, so in a child, after the in-process cases
WAVES12 = [(3, 13), (3, 25), (3, 36), (5, 13), (5, 25), (5, 36)]
CHILD = """
import test_gpu_abandon_edges as ae
out = {}
for band, L in ae.WAVES12:
    # dtw_mfma_abandon_kernel<5, 12, false, 8, true>; assertions (1) to (6) in here
    case, ws = ae.run_case(ra, ctx, "f32_matrix K5 T8 L%d band%d waves12" % (L, band), "mfma8", ([ae.MFMA], ["bf16x3"], [12]), 5, [L] * 8, band)
    for k, v in ws.items():
        out["b%d_L%d_%s" % (band, L, k)] = v
out["shares"] = np.array(["%s|%s|%s|%r|%r" % s for s in ae.SHARES])
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
def test_twelve_wave_abandon_build_in_a_child(ra, ctx, tmp_path):
    """RP_MFMA3_WAVES=12 launches dtw_mfma_abandon_kernel<5, 12, false, 8, true> for a detect-only call.  The child holds it to assertions
    (1) to (6); here its workspace equals the eight-wave build's wherever BOTH are non-zero -- which waves die may differ between the builds
    (a workgroup's waves share tiles differently), what a surviving DTW scores may not."""
    import child_runs
    mine = {}
    for band, L in WAVES12:
        _, ws = run_case(ra, ctx, "f32_matrix K5 T8 L%d band%d" % (L, band), "mfma8", X_MFMA8, 5, [L] * 8, band, record=False)   # (recorded above)
        for k, v in ws.items():
            mine["b%d_L%d_%s" % (band, L, k)] = v
    theirs = child_runs.run_each(tmp_path, CHILD, [("waves12", {"RP_MFMA3_WAVES": "12"})], timeout=120)["waves12"]
    for line in theirs.pop("shares"):
        name, route, thr_name, thr, share = str(line).split("|")
        SHARES.append((name, route, thr_name, float(thr), float(share)))
    assert sorted(theirs) == sorted(mine)
    for k in mine:
        a, b = _bits(mine[k]), _bits(theirs[k])
        both = (a != 0) & (b != 0)
        assert np.array_equal(a[both], b[both]), k
        if "t999" not in k:
            assert both.any(), k


# ------------------------------------------------------------------ the record
@pytest.mark.gpu
def test_write_the_abandoned_shares():
    """Runs last: what share of the DTWs each case abandoned at each threshold, for profiles/abandon_edges.txt.  100 % at 0.999 for every
    checked length, 0 % for the never-checked ones and non-zero at q99 are asserted where they are measured (check_case)."""
    path = os.environ.get("RP_ABANDON_EDGES_PROFILE")
    if not path or not SHARES:
        return
    with open(path, "w") as f:
        f.write("# tests/test_gpu_abandon_edges.py on one MI355X: %.1f s from the first case to this line (%d cases x thresholds)\n" % (time.time() - _T0[0], len(SHARES)))
        f.write("# case | checks as | threshold | share of the call's DTWs abandoned (score 0 in the workspace)\n")
        for name, route, thr_name, thr, share in SHARES:
            f.write("%-46s %-7s %-5s %.6f  %7.3f %%\n" % (name, route, thr_name, thr, 100.0 * share))
