"""Wakeword banks at the places where the kernels can go wrong unseen (tests/test_gpu_wakeword_bank.py covers the golden wakewords): every
dtw_bank_kernel<K, W> build at the lengths next to its unroll edges, three tiles at mfcc_size 13 / 16, every score mode, more than 64 KB
of LDS up to the largest wakeword a bank accepts, waves in which only some lanes take the reference-shaped cell, device-pointer contexts,
130 streams through scan_bank_kernel, a wakeword's own thresholds, and the small corners of the API.

Two witnesses throughout: the CPU oracle at the project's parity bar (relative error <= 1e-5), and bit equality with the per-wakeword
path -- rp_dtw_score_batch / rp_batch_detect under RP_ARITH_STRICT_F32 with the wakeword as rp_templates -- which include/rustpotter_hip.h
promises."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rpw_py
from oracle import rp_oracle as orc
from test_gpu_wakeword_bank import (G, GOLDEN_RPW, SEED, Wakeword, bits, check_against_per_wakeword, ctx, golden, golden_streams,  # noqa: F401
                                    oracle_frames, ra, read, rel_err)

pytestmark = pytest.mark.gpu


def mode_name(mode):
    return mode.name.lower()   # ScoreMode.P90 -> the oracle's "p90"


def oracle_rows(mf_s, ww, band):
    """the oracle's scores of one stream against one wakeword: [n_win][T] per sample template, [n_win] of the averaged template (or None)"""
    sc, _ = orc.score_stream(mf_s, ww.templates, band=band)
    n_win = sc.shape[0]
    av = None
    if ww.avg is not None:
        av = np.array([orc.score_window(mf_s[w:w + ww.max_len], ww.avg, band=band) for w in range(n_win)], np.float32)
    return sc, av


def check_scores(ra, ctx, bank, wws, mf, idx, band, modes, win_pitch=None):
    """rp_dtw_score_bank over mf [S][nf][K]: per stream agg / avg within 1e-5 of the oracle and bit-equal to rp_dtw_score_batch under strict
    f32 with its wakeword as rp_templates; zero rows without a wakeword, zeros behind a stream's windows.  A wakeword of one-frame templates
    only has no DTW row at all: exactly the oracle's value, the logistic of an infinite cost.  -> worst relative error against the oracle"""
    S, nf, _ = mf.shape
    idx = np.asarray(idx, np.int32)
    refs = {s: oracle_rows(mf[s], wws[idx[s]], band) for s in range(S) if idx[s] >= 0 and nf >= wws[idx[s]].max_len}
    worst = 0.0
    for mode in modes:
        ctx.dtw_kernels()
        avg, agg = ctx.dtw_scores_bank(mf, bank, idx, band_size=band, score_mode=mode, with_avg=True, win_pitch=win_pitch)
        assert ctx.dtw_kernels() == ["dtw_bank_kernel"]
        for s in range(S):
            if idx[s] < 0:
                assert not agg[s].any() and not avg[s].any(), (mode, s)
                continue
            ww = wws[idx[s]]
            n_win = max(0, nf - ww.max_len + 1)
            assert not agg[s][n_win:].any() and not avg[s][n_win:].any(), (mode, s, "rows behind n_win are zero")
            if n_win == 0:
                continue
            ref_sc, ref_v = refs[s]
            ref_a = np.array([orc.aggregate(r, mode_name(mode)) for r in ref_sc], np.float32)
            e = rel_err(agg[s][:n_win], ref_a)
            worst = max(worst, e)
            assert e <= 1e-5, (mode, s, e)
            if ww.max_len == 1:
                assert np.isfinite(agg[s][:n_win]).all() and np.array_equal(agg[s][:n_win], ref_a) and not ref_a.any(), (mode, s)
            with ctx.arithmetic("strict_f32"):
                _, b_avg, b_agg = ctx.dtw_scores(mf[s], ww.t, band_size=band, score_mode=mode, with_avg=ww.avg is not None)
            diff = bits(agg[s][:n_win]) != bits(b_agg[0])
            assert not diff.any(), (mode, s, "agg differs from the per-wakeword call in windows", np.flatnonzero(diff)[:8])
            if ww.avg is not None:
                e = rel_err(avg[s][:n_win], ref_v)
                worst = max(worst, e)
                assert e <= 1e-5, (mode, s, "avg", e)
                assert np.array_equal(bits(avg[s][:n_win]), bits(b_avg[0])), (mode, s, "avg")
            else:
                assert not avg[s].any(), (mode, s)
    return worst


def synth(seed, L, K):
    return orc.synth_templates(SEED + seed, 1, L, K)[0]


def averaged(templates):
    return orc.average_templates({"t%02d" % t: x for t, x in enumerate(templates)})


@pytest.mark.parametrize("band", [3, 4, 5, 6])
@pytest.mark.parametrize("K", [5, 13, 16])
def test_every_build_at_the_unroll_edges(ra, ctx, K, band):
    """1. dtw_bank_kernel<K, W> for all twelve (K, W): the guarded block is rows 1..2W, the unrolled loop starts at row 1 + 2W, columns
    1..W-1 are loaded before the first row.  Template lengths 1, 2, W, W+1, 2W, 2W+1, 2W+2, 4W, 4W+1 alone, and a very short template
    next to a long one (the window is cut to the short one's oldest frames); averaged templates as long as the window and shorter."""
    W = band
    single = [1, 2, W, W + 1, 2 * W, 2 * W + 1, 2 * W + 2, 4 * W, 4 * W + 1]
    mixed = [[1, 4 * W + 1], [4 * W + 3, 2], [W, 4 * W + 9, 2 * W + 1], [2, 70], [W + 1, 1, 2 * W + 2]]
    wws = []
    for w, lens in enumerate([[L] for L in single] + mixed):
        tm = [synth(100 * K + 10 * w + t, L, K) for t, L in enumerate(lens)]
        avg = None
        if lens == mixed[0] or lens == mixed[3]:
            avg = averaged(tm)                 # as long as the window
        if lens == mixed[2]:
            avg = averaged([tm[0], tm[2]])     # 2W+1 frames under a window of 4W+9
        wws.append(Wakeword(ra, ctx, tm, avg))
    bank = ra.WakewordBank(ctx, wakewords=[(w.templates, w.avg, None, None) for w in wws])
    assert bank.max_len == 70 and bank.max_lens[:9] == single
    nf = 73
    idx = list(range(len(wws)))
    idx.insert(5, -1)
    assert bank.n_win(nf, [0, 12]) == [73, 4]   # more than one tile for the shortest window, a handful for the longest
    mf = oracle_frames(len(idx), nf, K, 1200)
    worst = check_scores(ra, ctx, bank, wws, mf, idx, band, [ra.ScoreMode.Max, ra.ScoreMode.Average])
    print("K %d band %d: worst relative error against the oracle %.3g" % (K, band, worst))


@pytest.mark.parametrize("K", [13, 16])
def test_three_tiles_at_the_wide_frames(ra, ctx, K):
    """2. One call whose streams have exactly 64, 65, 129 and 0 windows at mfcc_size 13 / 16 (staging pitch 13 / 17): a full tile followed by
    an empty one, one window in the second tile, one in the third, and a stream shorter than its window."""
    nf, band = 140, 5
    shapes = [([77, 50], True), ([76], False), ([12, 9], True), ([150, 20], False)]
    wws = []
    for w, (lens, with_avg) in enumerate(shapes):
        tm = [synth(2000 + 100 * K + 10 * w + t, L, K) for t, L in enumerate(lens)]
        wws.append(Wakeword(ra, ctx, tm, averaged(tm) if with_avg else None))
    bank = ra.WakewordBank(ctx, wakewords=[(w.templates, w.avg, None, None) for w in wws])
    idx = [0, 1, 2, 3, -1, 2]
    assert bank.n_win(nf, idx) == [64, 65, 129, 0, 0, 129]
    mf = oracle_frames(len(idx), nf, K, 1300)
    worst = check_scores(ra, ctx, bank, wws, mf, idx, band, [ra.ScoreMode.Max, ra.ScoreMode.Average])
    print("K %d three tiles: worst relative error against the oracle %.3g" % (K, worst))


def test_every_score_mode(ra, ctx):
    """3. All nine score modes with 1, 2, 5 and 32 sample templates: T = 1 reads index 0, T = 2 is pure interpolation, T = 32 fills the
    last row of the percentile block (next to the band of the reference-shaped cell); two of the 32 are the same template, so the sort meets ties."""
    K, band, nf = 5, 5, 100
    rng = np.random.default_rng(33)
    wws = []
    for w, T in enumerate([1, 2, 5, 32]):
        lens = [int(x) for x in rng.integers(12, 31, T)]
        tm = [synth(3000 + 40 * w + t, L, K) for t, L in enumerate(lens)]
        if T == 32:
            tm[20] = tm[7].copy()
        wws.append(Wakeword(ra, ctx, tm, None))
    bank = ra.WakewordBank(ctx, wakewords=[(w.templates, None, None, None) for w in wws])
    idx = [0, 1, 2, 3, 3]
    mf = oracle_frames(len(idx), nf, K, 1400)
    modes = list(ra.ScoreMode)
    assert sorted(mode_name(m) for m in modes) == sorted(orc.SCORE_MODES)
    worst = check_scores(ra, ctx, bank, wws, mf, idx, band, modes)
    print("score modes: worst relative error against the oracle %.3g" % worst)


# ---- 4. LDS above 64 KB and the frame limit

def bank_lds_bytes(K, L):
    """dtw_bank_lds_bytes of rp_kernels.h: 64 + L + 6 staged frames of K | 1 floats, the percentile block [32][64], the band [13][64]"""
    return ((64 + L + 6) * (K | 1) + 32 * 64 + 13 * 64) * 4


def register_staged(K, L):
    """dtw_register_staged of rp_kernels.h: two tiles of 64 windows + two window lengths (+ 8) of frames in 160 KB"""
    return (2 * 64 + 2 * (L + 8)) * (K | 1) * 4 <= 160 * 1024


def frame_limit(K):
    L = (160 * 1024 - (32 * 64 + 13 * 64) * 4) // ((K | 1) * 4) - 70
    assert bank_lds_bytes(K, L) <= 160 * 1024 < bank_lds_bytes(K, L + 1)
    return L


@pytest.mark.parametrize("K,lim", [(5, 7546), (13, 2859), (16, 2170)])
def test_frame_limit_and_its_message_agree(ra, ctx, K, lim):
    """4a. Bank::create refuses a wakeword whose launch would need more than 160 KB of LDS and names a limit from a formula of its own: the
    limit it prints is the longest wakeword it accepts, and both follow from dtw_bank_lds_bytes."""
    assert frame_limit(K) == lim
    staged = {5: 4024, 13: 1503, 16: 1132}[K]   # the longest window the register kernels stage: below the bank's limit at every size
    assert register_staged(K, staged) and not register_staged(K, staged + 1) and staged < lim
    t = np.random.default_rng(K).standard_normal((lim + 1, K)).astype(np.float32)
    with pytest.raises(ra.RustpotterError, match=r"^wakeword 0: wakeword template of %d frames is too long" % (lim + 1)) as e:
        ra.WakewordBank(ctx, wakewords=[([t], None, None, None)])
    m = re.search(r"\(limit (\d+) frames at mfcc_size (\d+)\)", str(e.value))
    assert m and (int(m.group(1)), int(m.group(2))) == (lim, K), str(e.value)
    assert ra.WakewordBank(ctx, wakewords=[([t[:lim]], None, None, None)]).max_len == lim


def f64_band_scores(mf, tpl, band, score_ref=0.22):
    """f64_scores of tests/test_gpu_dtw_f64.py for one template of any length: the same formula in double precision from the f32 inputs,
    with the band kept as 2W + 1 running values per window instead of the whole (m+1) x (n+1) matrix.  -> [n_win]"""
    x, a = np.asarray(mf, np.float64), np.asarray(tpl, np.float64)
    m = a.shape[0]
    n_win = x.shape[0] - m + 1
    mu = np.stack([x[w:w + m].sum(axis=0) / m for w in range(n_win)])
    na = (a * a).sum(axis=1)
    P = np.full((2 * band + 2, n_win), np.inf)   # P[q] = D[r-1][r-1-W+q]
    P[band] = 0.0
    for r in range(1, m):
        left = np.full(n_win, np.inf)
        for q in range(2 * band):
            c = r - band + q
            v = np.full(n_win, np.inf)
            if 1 <= c <= m:
                y = x[c - 1:c - 1 + n_win] - mu
                mag = np.sqrt(na[r - 1] * (y * y).sum(axis=1))
                cos = np.where(mag == 0.0, 0.0, (y @ a[r - 1]) / np.where(mag == 0.0, 1.0, mag))
                v = (1.0 - cos) + np.minimum(np.minimum(P[q + 1], left), P[q])
            P[q] = v
            left = v
    nc = P[band + 1] / (m + m)
    return 1.0 / (1.0 + np.exp((nc - score_ref) / score_ref))


def test_f64_band_restatement_agrees_with_f64_scores():
    """the rolling-band f64 evaluation above is f64_scores of tests/test_gpu_dtw_f64.py (the whole matrix) on a short template"""
    from test_gpu_dtw_f64 import f64_scores
    rng = np.random.default_rng(8)
    mf = rng.standard_normal((40, 16)).astype(np.float32)
    for L in (1, 2, 7, 23):
        t = rng.standard_normal((L, 16)).astype(np.float32)
        want = f64_scores(mf, [t], band=5)[:, 0]
        got = f64_band_scores(mf, t, 5)
        assert np.allclose(got, want, rtol=1e-12, atol=0), L


def parity_or_f32_grade(got, ref, tru, what):
    """The parity bar against the f32 oracle, 1e-5.  Where sums of thousands of cell costs put the oracle's own rounding near that bar, the
    measure is the one of tests/test_gpu_dtw_f64.py for an f32-grade evaluation: the kernel is at most 1.25 x as far from the f64 value of
    the same formula as the oracle is.  `tru` computes the f64 scores and is only called when the bar is missed."""
    e = rel_err(got, ref)
    print("%s: relative error against the oracle %.3g" % (what, e))
    if e <= 1e-5:
        return e
    t = tru()
    d_orc, d_ker = rel_err(ref, t), rel_err(got, t)
    print("%s: largest distance from f64 -- oracle %.3g, kernel %.3g (ratio %.3f)" % (what, d_orc, d_ker, d_ker / d_orc))
    assert d_ker <= 1.25 * d_orc, (what, e, d_orc, d_ker)
    return e


@pytest.mark.parametrize("L", [725, 2170])
def test_long_wakewords_above_64_kb_of_lds(ra, ctx, L):
    """4b. mfcc_size 16: L = 725 is the first wakeword whose launch needs more than 64 KB of dynamic LDS, L = 2170 the largest a bank accepts
    (160 KB exactly: the percentile block and the band of the reference-shaped cell end at the top of LDS).  70 windows in two tiles; one
    ordinary stream, and one with a single frame near its end scaled by 1e17, so that the last windows take the reference-shaped cell there.
    Measured on an MI355X: the largest relative error against the oracle is 4.6e-7 at both lengths, so the 1e-5 bar holds at 2 170 rows
    and the f64 measure of parity_or_f32_grade is not needed.  L = 2 170 is past what the register kernels stage (1 132 frames here), so
    rp_templates scores it with dtw_generic_kernel, which range-tests a window's own frames only, and so does the bank
    (BankWakeword::window_chk) -- in every call shape: the same comparison once more with two streams of 21 windows, where a staged
    window is read from global memory by the register kernels."""
    K, band = 16, 5
    assert bank_lds_bytes(K, 724) <= 64 * 1024 < bank_lds_bytes(K, 725) and frame_limit(K) == 2170
    rng = np.random.default_rng(L)
    tm = [rng.standard_normal((n, K)).astype(np.float32) for n in (L, L - 3)]
    tm = [t - t.mean(axis=0, dtype=np.float32) for t in tm]
    ww = Wakeword(ra, ctx, tm, averaged(tm))
    assert ww.avg.shape[0] == L
    bank = ra.WakewordBank(ctx, wakewords=[(ww.templates, ww.avg, None, None)])
    nf = L + 69
    mf = rng.standard_normal((2, nf, K)).astype(np.float32)
    hot = nf - 5
    mf[1, hot] = (mf[1, hot].astype(np.float64) * 1e17).astype(np.float32)
    all_slow = hot - L + 1   # the first window that holds the frame; a template of L' rows loads frames w .. w + L' + W - 3
    n_win = 70
    before = ctx.dtw_ref_pairs()
    ctx.dtw_kernels()
    avg, agg = ctx.dtw_scores_bank(mf, bank, [0, 0], band_size=band, with_avg=True)
    assert ctx.dtw_kernels() == ["dtw_bank_kernel"] and agg.shape == (2, n_win)
    pairs = ctx.dtw_ref_pairs() - before
    assert np.isfinite(agg).all() and np.isfinite(avg).all() and agg.min() > 0
    # A template of L' rows loads frames w .. w + L' + W - 3 of window w: the windows that hold the scaled frame or load it behind their end
    # take the reference-shaped cell -- up to the window length the register kernels stage (dtw_register_staged: 1132 frames here).  A longer
    # window goes to dtw_generic_kernel as rp_templates, which loads the window's own frames only: then those of the bank must do the same.
    staged = register_staged(K, L)
    assert staged == (L == 725) and register_staged(K, 1132) and not register_staged(K, 1133)
    assert pairs == sum(n_win - max(0, hot - (n + (band - 3 if staged else -1))) for n in (L, L - 3, L)), pairs
    with ctx.arithmetic("strict_f32"):
        before = ctx.dtw_ref_pairs()
        _, b_avg, b_agg = ctx.dtw_scores(mf, ww.t, band_size=band, with_avg=True)
        assert ctx.dtw_ref_pairs() - before == pairs
        assert ctx.dtw_kernels() == (["register kernels"] if staged else ["dtw_generic_kernel"])
    assert np.array_equal(bits(agg), bits(b_agg)) and np.array_equal(bits(avg), bits(b_avg))
    # fewer than 64 windows in more than one stream: the route of live-stream batches
    few = np.ascontiguousarray(mf[:, nf - (L + 20):])
    before = ctx.dtw_ref_pairs()
    f_avg, f_agg = ctx.dtw_scores_bank(few, bank, [0, 0], band_size=band, with_avg=True)
    f_pairs = ctx.dtw_ref_pairs() - before
    assert f_agg.shape == (2, 21) and f_pairs == sum(21 - max(0, L + 15 - (n + (band - 3 if staged else -1))) for n in (L, L - 3, L)), f_pairs
    with ctx.arithmetic("strict_f32"):
        before = ctx.dtw_ref_pairs()
        ctx.dtw_kernels()
        _, b_avg, b_agg = ctx.dtw_scores(few, ww.t, band_size=band, with_avg=True)
        assert ctx.dtw_ref_pairs() - before == f_pairs
        assert ctx.dtw_kernels() == (["register kernels"] if staged else ["dtw_generic_kernel"])
    assert np.array_equal(bits(f_agg), bits(b_agg)) and np.array_equal(bits(f_avg), bits(b_avg))
    assert np.array_equal(bits(f_agg), bits(agg[:, 49:])) and np.array_equal(bits(f_avg), bits(avg[:, 49:])), "a window's bits do not depend on the call's shape"
    for s in range(2):
        ref_sc, ref_v = oracle_rows(mf[s], ww, band)
        ref_a = ref_sc.max(axis=1)
        n_ord = n_win if s == 0 else all_slow
        tru_sc = {}

        def tru(t):
            if t not in tru_sc:
                tru_sc[t] = f64_band_scores(mf[s], (tm + [ww.avg])[t], band)[:n_ord]
            return tru_sc[t]
        parity_or_f32_grade(agg[s][:n_ord], ref_a[:n_ord], lambda: np.maximum(tru(0), tru(1)), "L %d stream %d agg" % (L, s))
        parity_or_f32_grade(avg[s][:n_ord], ref_v[:n_ord], lambda: tru(2), "L %d stream %d avg" % (L, s))
        if s == 1:   # the windows that hold the scaled frame: the reference's own cell, operation for operation
            e = max(rel_err(agg[s][n_ord:], ref_a[n_ord:]), rel_err(avg[s][n_ord:], ref_v[n_ord:]))
            print("L %d stream 1, windows on the reference-shaped cell: relative error against the oracle %.3g" % (L, e))
            assert e <= 1e-5, e


# ---- 5. waves in which some lanes take the reference-shaped cell

@pytest.mark.parametrize("K", [5, 13])
def test_mixed_waves_on_the_slow_path(ra, ctx, K):
    """5. One frame in mid-stream scaled by 1e17 (another stream: by 1e-20): some windows of a tile hold the frame, some only load it as a
    look-ahead column behind their end, the rest never see it -- `if (slow) sc = rs` with both kinds of lanes in one wave, with an averaged
    template, three sample templates, max and median.  Then a wakeword whose rows are scaled by 3e-23: every window takes that cell."""
    nf, band = 150, 5
    lens = (40, 33, 37)
    tm = [synth(5000 + 10 * K + t, L, K) for t, L in enumerate(lens)]
    ww = Wakeword(ra, ctx, tm, averaged(tm))
    small = [(t.astype(np.float64) * 3e-23).astype(np.float32) for t in tm + [ww.avg]]
    ww_small = Wakeword(ra, ctx, small[:3], small[3])
    wws = [ww, ww_small]
    bank = ra.WakewordBank(ctx, wakewords=[(w.templates, w.avg, None, None) for w in wws])
    mf = oracle_frames(3, nf, K, 1500)
    mf[0, 75] = (mf[0, 75].astype(np.float64) * 1e17).astype(np.float32)
    mf[1, 60] = (mf[1, 60].astype(np.float64) * 1e-20).astype(np.float32)
    n_win = nf - 40 + 1
    for mode in (ra.ScoreMode.Max, ra.ScoreMode.Median):
        before = ctx.dtw_ref_pairs()
        worst = check_scores(ra, ctx, bank, wws, mf, [0, 0, 0], band, [mode])
        both = ctx.dtw_ref_pairs() - before           # check_scores: one bank call, then one strict-f32 call per stream
        before = ctx.dtw_ref_pairs()
        ctx.dtw_scores_bank(mf, bank, [0, 0, 0], band_size=band, score_mode=mode, with_avg=True)
        mine = ctx.dtw_ref_pairs() - before
        assert both == 2 * mine, "the per-wakeword calls rescore the same (window, template) pairs"
        # a template of L rows loads frames w .. w + L + W - 3 of window w: the windows that hold the large frame or load it behind their end.
        # (The frame scaled down is as far from its window's mean as any other: it stays on the ordinary path.)
        expect = sum(75 - max(0, 75 - (L + band - 3)) + 1 for L in lens + (40,))
        assert mine == expect, (mine, expect)
        print("K %d %s mixed waves: %d pairs on the reference-shaped cell, worst relative error against the oracle %.3g" % (K, mode_name(mode), mine, worst))
    before = ctx.dtw_ref_pairs()
    ctx.dtw_scores_bank(mf[2:], bank, [1], band_size=band, with_avg=True)
    assert ctx.dtw_ref_pairs() - before == n_win * 4, "ref_only: every window against every template"
    worst = check_scores(ra, ctx, bank, wws, mf[2:], [1], band, [ra.ScoreMode.Max, ra.ScoreMode.Median])
    print("K %d ref_only wakeword: worst relative error against the oracle %.3g" % (K, worst))


# ---- 6. device pointers

def dev_call(torch, dctx, dbank, d_pcm, idx, cfg, max_det, pitch):
    """rp_batch_detect_bank on device arrays, every output pre-filled: det / n_det with -1 bytes, agg / avg (when pitch is given) with NaN"""
    S, N = d_pcm.shape
    d_idx = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).cuda()
    det = torch.full((S, max_det, 6), -1, dtype=torch.int32, device="cuda")
    n_det = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    agg = avg = None
    if pitch is not None:
        agg = torch.full((S, pitch), float("nan"), dtype=torch.float32, device="cuda")
        avg = torch.full((S, pitch), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dctx.batch_detect_bank_dev(d_pcm.data_ptr(), 3, S, N, N, dbank, d_idx.data_ptr(), cfg, det.data_ptr(), n_det.data_ptr(), max_det,
                               None if agg is None else agg.data_ptr(), None if avg is None else avg.data_ptr(), pitch or 0)
    dctx.synchronize()
    out = (det.cpu().numpy(), n_det.cpu().numpy())
    return out if agg is None else out + (agg.cpu().numpy(), avg.cpu().numpy())


def test_device_pointers(ra, ctx, golden, golden_streams):
    """6. A context that takes device pointers, with a bank of its own: results go straight into the caller's arrays, win_pitch must hold the
    bank-wide largest window count (from the bank's shortest window, whatever the call's streams use), and an index outside [0, W) is "no
    wakeword" in both kernels.  Every element of every row is written; rows and detections are the host-pointer context's, bit for bit."""
    import torch
    bank, _ = golden
    pcm, idx0 = golden_streams
    dctx = ra.BatchContext(device=0, host_pointers=False)
    dbank = ra.WakewordBank(dctx, rpw=[read(n) for n in GOLDEN_RPW])
    S, N = pcm.shape
    nf = ra.mfcc_num_frames(N)
    P = nf - min(bank.max_lens) + 1
    cfg = ra.DetectorConfig()
    MAXD = 4
    idx = np.array(idx0, np.int32)
    assert list(idx) == [0, 1, 2, 0, 1, 2, 0, 1, 2, -1]
    outside, none = idx.copy(), idx.copy()
    outside[[1, 3, 8]] = [bank.W, bank.W + 5, -7]
    none[[1, 3, 8]] = -1
    d_pcm = torch.from_numpy(pcm).cuda()
    for pitch in (P, P + 1, (P + 63) // 64 * 64 + 1):
        for given, same_as in ((idx, idx), (outside, none)):
            h_det, h_n, h_agg, h_avg = ctx.batch_detect_bank(pcm, bank, same_as, cfg, max_det=MAXD, want_agg=True, win_pitch=pitch)
            det, n_det, agg, avg = dev_call(torch, dctx, dbank, d_pcm, given, cfg, MAXD, pitch)
            assert not np.isnan(agg).any() and not np.isnan(avg).any(), "every element of every row is written"
            assert np.array_equal(bits(agg), bits(h_agg)) and np.array_equal(bits(avg), bits(h_avg)), pitch
            assert np.array_equal(n_det, h_n) and det.tobytes() == h_det.tobytes(), pitch
            for s in np.flatnonzero(same_as < 0):
                assert n_det[s] == 0 and not det[s].any() and not agg[s].any() and not avg[s].any(), (pitch, s)
        assert h_n[4] >= 1, "the golden detection is among them"
    # detect-only
    for given, same_as in ((idx, idx), (outside, none)):
        h_det, h_n = ctx.batch_detect_bank(pcm, bank, same_as, cfg, max_det=MAXD)
        det, n_det = dev_call(torch, dctx, dbank, d_pcm, given, cfg, MAXD, None)
        assert np.array_equal(n_det, h_n) and det.tobytes() == h_det.tobytes()
    # the pitch is checked against the bank, not against the call: wakeword 2 alone has fewer windows
    only2 = np.full(S, 2, np.int32)
    with pytest.raises(ra.RustpotterError, match=r"win_pitch %d is smaller than the largest window count of the call \(%d\)" % (P - 1, P)):
        dev_call(torch, dctx, dbank, d_pcm, only2, cfg, MAXD, P - 1)
    # rp_dtw_score_bank
    mf = ctx.mfcc(pcm, 5)
    d_mf = torch.from_numpy(mf).cuda()
    d_idx = torch.from_numpy(outside).cuda()
    for pitch in (P, P + 1, (P + 63) // 64 * 64 + 1):
        h_avg, h_agg = ctx.dtw_scores_bank(mf, bank, none, with_avg=True, win_pitch=pitch)
        d_agg = torch.full((S, pitch), float("nan"), dtype=torch.float32, device="cuda")
        d_avg = torch.full((S, pitch), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dctx.dtw_scores_bank_dev(d_mf.data_ptr(), S, nf, dbank, d_idx.data_ptr(), 0.22, 5, ra.ScoreMode.Max, True, d_avg.data_ptr(), d_agg.data_ptr(), pitch)
        dctx.synchronize()
        agg, avg = d_agg.cpu().numpy(), d_avg.cpu().numpy()
        assert not np.isnan(agg).any() and not np.isnan(avg).any()
        assert np.array_equal(bits(agg), bits(h_agg)) and np.array_equal(bits(avg), bits(h_avg)), pitch
    d_only2 = torch.from_numpy(only2).cuda()
    with pytest.raises(ra.RustpotterError, match=r"win_pitch %d is smaller than the largest window count of the call \(%d\)" % (P - 1, P)):
        dctx.dtw_scores_bank_dev(d_mf.data_ptr(), S, nf, dbank, d_only2.data_ptr(), 0.22, 5, ra.ScoreMode.Max, True, d_avg.data_ptr(), d_agg.data_ptr(), P - 1)


# ---- 7 / 8. detections against the oracle's detector

def oracle_detections(wdict, pcm, cfg):
    """orc.Detector = Rustpotter::new(config) + add_wakeword(wdict, with its own thresholds) + process_samples per 30 ms chunk"""
    d = orc.Detector(avg_threshold=cfg.avg_threshold, threshold=cfg.threshold, min_scores=cfg.min_scores, eager=cfg.eager,
                     score_ref=cfg.score_ref, band_size=cfg.band_size, score_mode=mode_name(cfg.score_mode))
    d.add_ref(wdict)
    out = []
    for i in range(0, len(pcm) - 479, 480):
        r = d.process_f32(pcm[i:i + 480])
        if r is not None:
            out.append((i // 480, r))
    return out


def check_against_oracle_detector(wdict, pcm, cfg, det_row, n, max_det):
    """frame (as the chunk it lies in), counter and window equal, score and avg_score within 1e-5.  The oracle's detector reports no window;
    the one the kernel reports must be a window whose oracle score IS the score the oracle's detector reports.  -> worst relative error"""
    want = oracle_detections(wdict, pcm, cfg)
    assert n == len(want) and n <= max_det, (n, want)
    templates = list(wdict["samples_features"].values())
    max_len = max(len(t) for t in templates)
    mfo = orc.mfcc_stream(pcm, templates[0].shape[1]) if n else None
    worst = 0.0
    for j, (chunk, r) in enumerate(want):
        d = det_row[j]
        assert d["frame"] // 3 + 1 == chunk and d["counter"] == r["counter"], (j, d, chunk, r)
        w = int(d["window"])
        sc = [orc.score_window(mfo[w:w + max_len], t, band=cfg.band_size, score_ref=cfg.score_ref) for t in templates]
        assert np.float32(orc.aggregate(sc, mode_name(cfg.score_mode))) == r["score"], (j, "window", w)
        e = abs(float(d["score"]) - float(r["score"])) / float(r["score"])
        if r["avg_score"] == 0:
            assert d["avg_score"] == 0
        else:
            e = max(e, abs(float(d["avg_score"]) - float(r["avg_score"])) / float(r["avg_score"]))
        assert e <= 1e-5, (j, d, r)
        worst = max(worst, e)
    return worst


def test_130_streams_through_both_kernels(ra, ctx, golden, golden_streams):
    """7. S = 130: two full blocks of scan_bank_kernel and one of two lanes; the golden recordings against a seeded permutation of the golden
    wakewords and "none".  As one call per wakeword; one stream per (recording, wakeword) also against the oracle's detector with that
    wakeword's own thresholds.  Stream 128, in the partial block, is oye_casa_g_1.wav with oye_casa_g.rpw and must fire.  Nothing carries
    over between calls on one context: quiet streams next report nothing, then the first call again gives identical bytes.  (That does not
    observe the per-stream `hot` flags: the scan only uses them to skip a stream, and a flag left raised makes it read a row this call has
    rewritten -- it would cost time, not results.)  A context with RP_CTX_FULL_SCORES finds the same."""
    bank, wws = golden
    pcm10, _ = golden_streams
    S, MAXD = 130, 4
    idx = np.random.default_rng(130).permutation(np.resize(np.array([-1, 0, 1, 2], np.int32), S)).astype(np.int32)
    rec = (np.arange(S) + 2) % 3          # stream 128 is the oye_casa recording
    j = int(np.flatnonzero((idx == 1) & (np.arange(S) < 128))[-1])
    idx[j], idx[128] = idx[128], 1
    pcm = np.ascontiguousarray(pcm10[[0, 3, 6]][rec])
    first = {}
    for s in range(S):
        first.setdefault((int(rec[s]), int(idx[s])), s)
    first[(1, 1)] = 128                   # the one that fires, from the partial block, also against the oracle's detector
    assert len(first) == 12 and (idx[:64] >= 0).any() and (idx[64:128] >= 0).any() and rec[128] == 1 and idx[128] == 1
    cfg = ra.DetectorConfig()
    det, n_det = check_against_per_wakeword(ra, ctx, bank, wws, pcm, idx, cfg, max_det=MAXD, want_agg=True)
    det_o, n_o = check_against_per_wakeword(ra, ctx, bank, wws, pcm, idx, cfg, max_det=MAXD, want_agg=False)
    assert np.array_equal(n_o, n_det) and det_o.tobytes() == det.tobytes()
    assert n_det[128] >= 1 and all(n_det[s] >= 1 for s in range(S) if rec[s] == 1 and idx[s] == 1), "oye_casa_g_1.wav against oye_casa_g.rpw"
    worst = 0.0
    for (_, w), s in sorted(first.items()):
        if w >= 0:
            wdict = rpw_py.load_rpw(os.path.join(G, GOLDEN_RPW[w]))
            worst = max(worst, check_against_oracle_detector(wdict, pcm[s], cfg, det[s], int(n_det[s]), MAXD))
    print("S = 130: n_det sum %d, worst relative error of a detection's scores against the oracle's detector %.3g" % (int(n_det.sum()), worst))
    # nothing carries over
    det_q, n_q = ctx.batch_detect_bank(np.zeros_like(pcm), bank, idx, cfg, max_det=MAXD)
    assert not n_q.any() and not det_q.tobytes().strip(b"\0")
    det_r, n_r = ctx.batch_detect_bank(pcm, bank, idx, cfg, max_det=MAXD)
    assert np.array_equal(n_r, n_det) and det_r.tobytes() == det.tobytes()
    fctx = ra.BatchContext(device=0, host_pointers=True, full_scores=True)
    fbank = ra.WakewordBank(fctx, rpw=[read(n) for n in GOLDEN_RPW])
    det_f, n_f = fctx.batch_detect_bank(pcm, fbank, idx, cfg, max_det=MAXD)
    assert np.array_equal(n_f, n_det) and det_f.tobytes() == det.tobytes()


def test_own_thresholds_against_the_oracle_detector(ra, ctx, golden_streams):
    """8. rp_wakeword_bank_new with explicit thresholds: four copies of oye_casa_g.rpw with (None, None), (0.45, None), (None, 0.0) and
    (None, 0.3) as their own (threshold, avg_threshold) -- and one with (None, 0.7), above the averaged template's score where the others
    fire -- under a config avg_threshold of 0.2 and of 0.0; every recording against every copy, checked against orc.Detector holding the
    same Options.  An effective avg_threshold of 0.0 switches the averaged template off: avg rows
    are zero and avg_score is 0 (wakeword_comp.rs:85)."""
    pcm10, _ = golden_streams
    base = rpw_py.load_rpw(os.path.join(G, "oye_casa_g.rpw"))
    templates, avg = list(base["samples_features"].values()), base["avg_features"]
    assert avg is not None
    own = [(None, None), (0.45, None), (None, 0.0), (None, 0.3), (None, 0.7)]
    bank = ra.WakewordBank(ctx, wakewords=[(templates, avg, t, a) for t, a in own])
    idx = np.array([c for c in range(len(own)) for _ in range(3)], np.int32)
    pcm = np.ascontiguousarray(pcm10[[0, 3, 6] * len(own)])
    MAXD = 4
    worst, fired = 0.0, 0
    for cfg_avg in (0.2, 0.0):
        cfg = ra.DetectorConfig()
        cfg.avg_threshold = cfg_avg
        det, n_det, agg, avgr = ctx.batch_detect_bank(pcm, bank, idx, cfg, max_det=MAXD, want_agg=True)
        det_o, n_o = ctx.batch_detect_bank(pcm, bank, idx, cfg, max_det=MAXD)
        assert np.array_equal(n_o, n_det) and det_o.tobytes() == det.tobytes()
        for s in range(len(idx)):
            t, a = own[idx[s]]
            wdict = dict(base, threshold=t, avg_threshold=a)
            worst = max(worst, check_against_oracle_detector(wdict, pcm[s], cfg, det[s], int(n_det[s]), MAXD))
            if (cfg_avg if a is None else a) == 0.0:
                assert not avgr[s].any() and not det[s]["avg_score"].any(), (cfg_avg, s)
            else:
                assert avgr[s].any(), (cfg_avg, s)
        assert n_det[[1, 4, 7, 10]].all(), "oye_casa_g_1.wav fires under each of the first four"
        fired += int(n_det.sum())
    print("own thresholds: %d detections, worst relative error against the oracle's detector %.3g" % (fired, worst))


def test_corners(ra, ctx, golden, golden_streams):
    """9. agg without avg and the reverse on rp_batch_detect_bank; streams shorter than every window; an empty bank."""
    bank, _ = golden
    pcm10, idx10 = golden_streams
    pcm, idx = np.ascontiguousarray(pcm10[2:6]), np.array(idx10[2:6], np.int32)
    S, N = pcm.shape
    nf = ra.mfcc_num_frames(N)
    pitch = nf - min(bank.max_lens) + 1
    L = ra.load_library()
    c = ra.DetectorConfig()._c()

    def raw(want_agg, want_avg):
        det, n = np.zeros((S, 4), ra.api.DET_DTYPE), np.zeros(S, np.int32)
        agg = np.full((S, pitch), np.nan, np.float32) if want_agg else None
        avg = np.full((S, pitch), np.nan, np.float32) if want_avg else None
        r = L.rp_batch_detect_bank(ctx._h, pcm.ctypes.data, 3, S, N, N, bank._h, idx.ctypes.data, C.byref(c), det.ctypes.data, n.ctypes.data, 4,
                                   None if agg is None else agg.ctypes.data, None if avg is None else avg.ctypes.data, pitch)
        assert r == 0, L.rp_last_error()
        return det, n, agg, avg
    det, n, agg, avg = raw(True, True)
    assert n[2] >= 1 and not np.isnan(agg).any() and not np.isnan(avg).any()
    det_a, n_a, agg_a, _ = raw(True, False)
    det_v, n_v, _, avg_v = raw(False, True)
    assert np.array_equal(bits(agg_a), bits(agg)) and np.array_equal(bits(avg_v), bits(avg))
    assert det_a.tobytes() == det.tobytes() == det_v.tobytes() and np.array_equal(n_a, n) and np.array_equal(n_v, n)
    # shorter than every window
    short = pcm[:, :480 * 20]
    assert ra.mfcc_num_frames(short.shape[1]) < min(bank.max_lens)
    cfg = ra.DetectorConfig()
    d, n, agg, avg = ctx.batch_detect_bank(short, bank, idx, cfg, max_det=4, want_agg=True)
    assert agg.shape == (S, 0) and not n.any() and not d.tobytes().strip(b"\0")
    d, n, agg, avg = ctx.batch_detect_bank(short, bank, idx, cfg, max_det=4, want_agg=True, win_pitch=5)
    assert not n.any() and not d.tobytes().strip(b"\0") and not agg.any() and not avg.any()
    d, n = ctx.batch_detect_bank(short, bank, idx, cfg, max_det=4)
    assert not n.any() and not d.tobytes().strip(b"\0")
    avg, agg = ctx.dtw_scores_bank(np.ones((S, 50, 5), np.float32), bank, idx, with_avg=True, win_pitch=3)
    assert not agg.any() and not avg.any()
    # an empty bank: a Rustpotter without wakewords
    for empty in (ra.WakewordBank(ctx, wakewords=[]), ra.WakewordBank(ctx, rpw=[])):
        assert empty.W == 0 and empty.max_len == 0
        none = np.full(S, -1, np.int32)
        d, n, agg, avg = ctx.batch_detect_bank(pcm, empty, none, cfg, max_det=4, want_agg=True, win_pitch=7)
        assert agg.shape == (S, 7) and not n.any() and not d.tobytes().strip(b"\0") and not agg.any() and not avg.any()
        d, n = ctx.batch_detect_bank(pcm, empty, none, cfg, max_det=4)
        assert not n.any() and not d.tobytes().strip(b"\0")
        avg, agg = ctx.dtw_scores_bank(np.ones((S, 50, 1), np.float32), empty, none, with_avg=True, win_pitch=7)
        assert agg.shape == (S, 7) and not agg.any() and not avg.any()
        with pytest.raises(ra.RustpotterError, match="wakeword index 0 is outside the bank"):
            ctx.batch_detect_bank(pcm, empty, np.zeros(S, np.int32), cfg)
