"""Wakeword sets over whole recordings (rp_dtw_score_bank_sets / rp_batch_detect_bank_sets; dtw_set_kernel, scan_set_kernel): stream s holds
up to eight wakewords of a bank, as a Rustpotter with several add_wakeword calls.  The slot rows are checked bit for bit against
rp_dtw_score_bank, set_size 1 against rp_batch_detect_bank, uniform sets against rp_batch_detect_multi under RP_ARITH_STRICT_F32, and the
detections against the CPU oracle's detector with several add_ref at the project's bar (frame, window, counter and wakeword exact, scores
within 1e-5).  "Bit for bit" holds where neither side rescored a pair with the reference-shaped cosine: ctx.dtw_ref_pairs() must not move."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import pytest

import rpw_py
import test_gpu_stream_bank as sbk
from oracle import rp_oracle as orc

pytestmark = pytest.mark.gpu

G = sbk.G
GOLDEN_RPW = sbk.GOLDEN_RPW   # bank order alexa / oye_casa_g / oye_casa_real: windows of 126 / 108 / 168 frames
SETS = "dtw_set_kernel"
bits, bits1, quiet, recording, read = sbk.bits, sbk.bits1, sbk.quiet, sbk.recording, sbk.read


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


@pytest.fixture(scope="module")
def golden(ra, ctx):
    dicts = [rpw_py.load_rpw(os.path.join(G, n)) for n in GOLDEN_RPW]
    bank = ra.WakewordBank(ctx, rpw=[read(n) for n in GOLDEN_RPW])
    assert bank.max_lens == [126, 108, 168]
    return bank, dicts


def lmax_of(bank, row):
    return max([0] + [bank.max_lens[w] for w in row if 0 <= w < bank.W])


def detect_sets(ctx, bank, pcm, sets, cfg, max_det=16, want_agg=False):
    """rp_batch_detect_bank_sets -> per stream [(frame, window, counter, score bits, avg bits, bank index)], agg, avg"""
    res = ctx.batch_detect_bank_sets(pcm, bank, np.asarray(sets, np.int32), cfg, max_det=max_det, want_agg=want_agg)
    det, dww, n_det = res[0], res[1], res[2]
    out = []
    for s in range(len(sets)):
        assert n_det[s] <= max_det
        out.append([(int(d["frame"]), int(d["window"]), int(d["counter"]), bits1(d["score"]), bits1(d["avg_score"]), int(dww[s][i]))
                    for i, d in enumerate(det[s][:n_det[s]])])
        assert all(d["stream"] == s for d in det[s][:n_det[s]])
        assert not det[s][n_det[s]:].tobytes().strip(b"\0"), "slots behind a stream's detections are zero"
    return (out, res[3], res[4]) if want_agg else (out, None, None)


def padded(rng, rec, behind=36000, front=8000):
    """0.5 s of quiet, the recording, `behind` or more quiet samples, a whole number of 30 ms chunks"""
    n = 480 * ((front + len(rec) + behind + 479) // 480)
    return np.concatenate([quiet(rng, front), rec, quiet(rng, n - front - len(rec))])


def stack(rows):
    n = max(len(r) for r in rows)
    rng = np.random.default_rng(5)
    return np.stack([np.concatenate([r, quiet(rng, n - len(r))]) for r in rows])


# ---------------------------------------------------------------------------------------------- 1. slot rows

def check_slot_rows(ctx, bank, mf, sets, band, mode, score_ref=0.22):
    """every row (s, j) of rp_dtw_score_bank_sets = the first n_win_s values of rp_dtw_score_bank's row for wakeword set[s][j], zeros behind;
    an empty slot and a stream shorter than its window: zero rows.  Returns the windows compared."""
    S, nf, _ = mf.shape
    sets = np.asarray(sets, np.int32)
    used = sorted({int(w) for w in sets.ravel() if w >= 0})
    # one bank call gives every stream's row for every wakeword used: block u holds the S streams against used[u]
    ref_avg, ref_agg = ctx.dtw_scores_bank(np.tile(mf, (len(used), 1, 1)), bank, np.repeat(used, S), score_ref=score_ref, band_size=band,
                                           score_mode=mode, with_avg=True, win_pitch=nf)
    pitch = max(1, max(max(0, nf - lmax_of(bank, r) + 1) for r in sets)) + 3   # not a multiple of anything
    avg, agg = ctx.dtw_scores_bank_sets(mf, bank, sets, score_ref=score_ref, band_size=band, score_mode=mode, with_avg=True, win_pitch=pitch)
    assert agg.shape == avg.shape == (S, sets.shape[1], pitch)
    n = 0
    for s in range(S):
        L = lmax_of(bank, sets[s])
        n_win = max(0, nf - L + 1) if L else 0
        for j, w in enumerate(sets[s]):
            if w < 0:
                assert not agg[s, j].any() and not avg[s, j].any(), (s, j)
                continue
            r = used.index(int(w)) * S + s
            assert np.array_equal(bits(agg[s, j, :n_win]), bits(ref_agg[r, :n_win])), (s, j, int(w), nf)
            assert np.array_equal(bits(avg[s, j, :n_win]), bits(ref_avg[r, :n_win])), (s, j, int(w), nf)
            assert not agg[s, j, n_win:].any() and not avg[s, j, n_win:].any(), (s, j, "zeros follow")
            n += n_win
    return n


def test_slot_rows_golden_bank(ra, ctx, golden):
    """1a. The golden bank over three recordings: every slot row is the bank call's, for every pair and the triple, holes and duplicates."""
    bank, _ = golden
    rng = np.random.default_rng(11)
    pcm = stack([padded(rng, recording(n), behind=8000) for n in ("alexa.wav", "oye_casa_g_1.wav", "oye_casa_real_1.wav")])
    mf = ctx.mfcc(pcm, 5)
    before = ctx.dtw_ref_pairs()
    ctx.dtw_kernels()
    n = 0
    for sets in ([[0, 1, 2], [2, 1, 0], [1, -1, 1]], [[0, 2], [-1, 1], [-1, -1]], [[1], [2], [0]]):
        n += check_slot_rows(ctx, bank, mf, sets, 5, ra.ScoreMode.Max)
    assert SETS in ctx.dtw_kernels()
    assert ctx.dtw_ref_pairs() == before
    print("%d windows bit-equal" % n)


# rows over the synthetic bank of tests/test_gpu_stream_bank.py (22 wakewords of 1 .. 65 frames; 4 and 15: [64, 65]; 5 and 16: 32 templates of
# 20 .. 49 frames with an averaged template; 7: [40, 40]; 0: one frame): holes, a row of all -1, duplicates, the longest first and last
ROWS3 = [[4, 7, 0], [-1, 3, -1], [-1, -1, -1], [6, 6, 6], [5, 16, 21], [10, -1, 15], [0, 1, 2], [7, 4, -1], [13, 18, 9]]
ROWS8 = [[0, 1, 2, 3, 4, 5, 6, 7], [-1, -1, -1, -1, -1, -1, -1, 15], [8, 8, -1, 9, 10, 11, 12, 13], [21, 20, 19, 18, 17, 16, 15, 14]]
ROWS1 = [[4], [-1], [5], [0], [16]]


_SYNTH = {}


def synth_bank(ra, ctx, K):
    """the 22 wakewords of tests/test_gpu_stream_bank.py's synthetic bank (its SHAPES twice, the second copy of a wakeword with several
    templates and the 32-template ones with an averaged template), as a bank of THIS module's context"""
    if K not in _SYNTH:
        rng = np.random.default_rng(100 + K)
        wakewords = []
        for copy in range(2):
            for w, (T, lens) in enumerate(sbk.SHAPES):
                if lens is None:
                    lens = [int(x) for x in rng.integers(20, 50, T)]
                tm = [orc.synth_templates(sbk.SEED + 100000 * K + 1000 * copy + 50 * w + t, 1, L, K)[0] for t, L in enumerate(lens)]
                avg = None
                if T > 1 and (copy == 1 or T == 32):
                    avg = orc.average_templates(OrderedDict(("t%02d" % t, x) for t, x in enumerate(tm)))
                wakewords.append((tm, avg, None, None))
        _SYNTH[K] = ra.WakewordBank(ctx, wakewords=wakewords)
    return _SYNTH[K]


@pytest.mark.parametrize("K,band", [(K, b) for K in (5, 13, 16) for b in (3, 4, 5, 6)])
def test_slot_rows_ragged_banks(ra, ctx, K, band):
    """1b. Ragged synthetic banks at every (mfcc_size, band) the kernels are built for x Average / Max / Median (Median over the 32-template
    wakewords uses the percentile block), set_size 1, 3 and 8.  n_frames puts n_win_s of the streams whose window is 65 frames on the tile
    edges 1, 64, 65 and 130; at 50 frames those streams are shorter than their window although a 40-frame wakeword of their set would
    fit: all their rows are zero."""
    bank = synth_bank(ra, ctx, K)
    assert bank.max_lens[4] == 65 and bank.max_lens[7] == 40 and bank.max_lens[5] < 50
    mf_all = ctx.mfcc(ctx.synth_pcm(sbk.SEED, 3, len(ROWS3), 160 * (194 + 8)), K)
    assert mf_all.shape[1] >= 194
    before = ctx.dtw_ref_pairs()
    n = 0
    for mode in (ra.ScoreMode.Average, ra.ScoreMode.Max, ra.ScoreMode.Median):
        for nf in (50, 65, 128, 129, 194):
            mf = np.ascontiguousarray(mf_all[:, :nf])
            n += check_slot_rows(ctx, bank, mf, ROWS3, band, mode)
            if mode == ra.ScoreMode.Median or nf == 129:
                n += check_slot_rows(ctx, bank, mf[:len(ROWS8)], ROWS8, band, mode)
                n += check_slot_rows(ctx, bank, mf[:len(ROWS1)], ROWS1, band, mode)
    assert ctx.dtw_ref_pairs() == before
    print("K %d band %d: %d windows bit-equal" % (K, band, n))


def test_stream_shorter_than_its_window_reports_nothing(ra, ctx, golden):
    """1c. A bank of oye_casa_g (108 frames) and a 400-frame wakeword over a stream of 330 frames: [0, 1] has all-zero rows and no detection
    although oye_casa_g would fit and, alone, fires on this audio -- the reference's window never fills."""
    _, dicts = golden
    d = dicts[1]
    long_one = orc.synth_templates(sbk.SEED + 77, 1, 400, 5)[0]
    bank = ra.WakewordBank(ctx, wakewords=[(list(d["samples_features"].values()), d["avg_features"], d["threshold"], d["avg_threshold"]),
                                           ([long_one], None, None, None)])
    assert bank.max_lens == [108, 400]
    rng = np.random.default_rng(12)
    n = 160 * 335
    x = np.concatenate([quiet(rng, 1600), recording("oye_casa_g_1.wav"), quiet(rng, n)])[:n]
    assert ra.api.mfcc_num_frames(n) == 330
    det, agg, avg = detect_sets(ctx, bank, np.stack([x, x]), [[0, 1], [0, -1]], ra.DetectorConfig(), want_agg=True)
    assert agg.shape[2] == 330 - 108 + 1
    assert not agg[0].any() and not avg[0].any() and not det[0]
    assert agg[1, 0].any() and not agg[1, 1].any() and det[1] and det[1][0][5] == 0


# ---------------------------------------------------------------------------------------------- 2. set_size 1, uniform sets

@pytest.fixture(scope="module")
def golden_streams():
    rng = np.random.default_rng(31)
    names = ["alexa.wav", "oye_casa_g_1.wav", "oye_casa_real_1.wav", "oye_casa_g_2.wav", "oye_casa_real_2.wav"]
    rows = [padded(rng, recording(n)) for n in names] + [(0.1 * rng.standard_normal(40000)).astype(np.float32)]
    return stack(rows)


def test_set_size_one_equals_the_bank_call(ra, ctx, golden, golden_streams):
    """2. set_size 1 is rp_batch_detect_bank: detections, agg and avg, fully scored and detect-only."""
    bank, _ = golden
    idx = [0, 1, 2, 2, 1, -1]
    cfg = ra.DetectorConfig()
    before = ctx.dtw_ref_pairs()
    ref, r_agg, r_avg = sbk.whole(ctx, bank, golden_streams, idx, cfg, want_agg=True)
    det, agg, avg = detect_sets(ctx, bank, golden_streams, [[w] for w in idx], cfg, want_agg=True)
    det0, _, _ = detect_sets(ctx, bank, golden_streams, [[w] for w in idx], cfg)
    assert ctx.dtw_ref_pairs() == before
    assert [[d[:5] for d in v] for v in det] == ref and det0 == det and sum(len(v) for v in det) >= 3
    assert all(d[5] == idx[s] for s, v in enumerate(det) for d in v)
    assert np.array_equal(bits(agg[:, 0]), bits(r_agg)) and np.array_equal(bits(avg[:, 0]), bits(r_avg))


@pytest.mark.parametrize("sets", [[0, 1, 2], [2, 0], [1, 2, 1]])
def test_uniform_sets_equal_batch_detect_multi(ra, ctx, golden, golden_streams, sets):
    """3. Every stream holds the same set: the detections are rp_batch_detect_multi's under RP_ARITH_STRICT_F32 -- n_det, frame, window,
    counter, score and avg bits and the wakeword -- which checks the kernel's fold against propose_best."""
    bank, dicts = golden
    cfg = ra.DetectorConfig()
    S = golden_streams.shape[0]
    before = ctx.dtw_ref_pairs()
    det, _, _ = detect_sets(ctx, bank, golden_streams, [sets] * S, cfg)
    tms = [ra.Templates(ctx, list(dicts[w]["samples_features"].values()), dicts[w]["avg_features"]) for w in sets]
    with ctx.arithmetic("strict_f32"):
        m_det, m_ww, m_n = ctx.batch_detect_multi(golden_streams, tms, cfg, thresholds=[dicts[w]["threshold"] for w in sets],
                                                  avg_thresholds=[dicts[w]["avg_threshold"] for w in sets], max_det=16)
    assert ctx.dtw_ref_pairs() == before
    want = [[(int(d["frame"]), int(d["window"]), int(d["counter"]), bits1(d["score"]), bits1(d["avg_score"]), sets[int(m_ww[s][i])])
             for i, d in enumerate(m_det[s][:m_n[s]])] for s in range(S)]
    assert det == want, (det, want)
    assert sum(len(v) for v in det) >= 3


# ---------------------------------------------------------------------------------------------- 4. the oracle

def oracle_sets(dicts, row, pcm, cfg):
    """orc.Detector = Rustpotter::new(config) + add_wakeword per live slot in slot order + process_samples per 30 ms chunk"""
    d = orc.Detector(avg_threshold=cfg.avg_threshold, threshold=cfg.threshold, min_scores=cfg.min_scores, eager=cfg.eager,
                     score_ref=cfg.score_ref, band_size=cfg.band_size, score_mode=sbk.mode_name(cfg.score_mode))
    for w in row:
        if w >= 0:
            d.add_ref(dicts[w])
    return [(i // 480, r) for i in range(0, len(pcm) - 479, 480) for r in [d.process_f32(pcm[i:i + 480])] if r is not None]


def same_as_oracle(dicts, bank, row, got, want):
    """frame (as its chunk), counter and wakeword (by its name and by the names of its templates) exact; score and avg score within 1e-5.  (The oracle reports no window: a detection's
    window is that of its best-scoring frame, Lmax(s) frames long and inside the stream, at or before the frame that emits it.)"""
    assert len(got) == len(want), (row, got, want)
    L = lmax_of(bank, row)
    for d, (chunk, r) in zip(got, want):
        assert d[0] // 3 + 1 == chunk and d[2] == r["counter"] and 0 <= d[1] <= d[0] - L + 1, (row, d, chunk, r)
        # the winner exactly: two golden wakewords share the name "oye casa", but the oracle's detection lists the winner's templates
        assert d[5] in row and dicts[d[5]]["name"] == r["name"], (row, d, r)
        assert sorted(r["scores"]) == sorted(dicts[d[5]]["samples_features"]), (row, d, sorted(r["scores"]))
        sc, av = np.array([d[3], d[4]], np.uint32).view(np.float32)
        assert abs(float(sc) - float(r["score"])) <= 1e-5 * float(r["score"]), (row, d, r)
        if r["avg_score"] == 0:
            assert av == 0
        else:
            assert abs(float(av) - float(r["avg_score"])) <= 1e-5 * float(r["avg_score"]), (row, d, r)


def test_sets_against_the_oracle(ra, ctx, golden):
    """4. The recordings and sets of the issue's table, both slot orders, and the two-utterance stream, against orc.Detector with add_ref in
    slot order.  [0, 2] on oye_casa_real_1 reports a larger counter than [2] alone (alexa proposes while the partial detection is open);
    [0, 1] on alexa + oye_casa_g_1 reports two detections by two different wakewords."""
    bank, dicts = golden
    rng = np.random.default_rng(41)
    real, g, alexa = recording("oye_casa_real_1.wav"), recording("oye_casa_g_1.wav"), recording("alexa.wav")
    two = np.concatenate([alexa, quiet(rng, 40000), g])
    plan = [(real, [2, -1]), (real, [0, 2]), (real, [2, 0]), (real, [0, 1]), (real, [1, 0]),
            (g, [1, -1]), (g, [0, 1]), (g, [1, 0]), (g, [1, 2]), (g, [2, 1]), (two, [0, 1]), (two, [1, 0])]
    pcm = stack([padded(rng, x) for x, _ in plan])
    sets = [r for _, r in plan]
    cfg = ra.DetectorConfig()
    before = ctx.dtw_ref_pairs()
    det, _, _ = detect_sets(ctx, bank, pcm, sets, cfg)
    assert ctx.dtw_ref_pairs() == before
    for s, row in enumerate(sets):
        same_as_oracle(dicts, bank, row, det[s], oracle_sets(dicts, row, pcm[s], cfg))
    print("detections (chunk, wakeword, counter):", [[(d[0] // 3 + 1, d[5], d[2]) for d in v] for v in det])
    assert len(det[0]) == 1 and len(det[1]) == 1 and det[1][0][2] > det[0][0][2] and det[1][0][3] == det[0][0][3] and det[1][0][5] == 2
    assert det[3] and det[3][0][5] == 0, "[0, 1] on oye_casa_real_1: alexa"
    assert det[5][0][0] < det[6][0][0] < det[8][0][0], "the window is as long as the set's longest wakeword: the detection comes later"
    for s in (10, 11):
        assert len(det[s]) == 2 and [d[5] for d in det[s]] == [0, 1], det[s]


# ---------------------------------------------------------------------------------------------- 5. tie, own thresholds, gate

def test_tie_names_the_first_slot(ra, ctx, golden_streams):
    """5. The same wakeword at two bank indices: equal scores, and the detection names the first slot's index, in both orders."""
    rpw = read("oye_casa_g.rpw")
    bank = ra.WakewordBank(ctx, rpw=[rpw, rpw])
    det, _, _ = detect_sets(ctx, bank, golden_streams[[1, 1]], [[0, 1], [1, 0]], ra.DetectorConfig())
    assert det[0] and [d[:5] for d in det[0]] == [d[:5] for d in det[1]]
    assert all(d[5] == 0 for d in det[0]) and all(d[5] == 1 for d in det[1])


def test_own_threshold_keeps_the_best_score_from_winning(ra, ctx, golden, golden_streams):
    """6. Wakeword 0 holds every template of oye_casa_g and a threshold of its own above all its scores; wakeword 1 holds all but one of them
    (ScoreMode::Max: never a higher score).  Wakeword 0 never wins although its scores are the highest, in both slot orders."""
    _, dicts = golden
    d = dicts[1]
    tm = list(d["samples_features"].values())
    assert len(tm) >= 2
    bank = ra.WakewordBank(ctx, wakewords=[(tm, d["avg_features"], 0.9999, d["avg_threshold"]), (tm[:-1], d["avg_features"], d["threshold"], d["avg_threshold"])])
    cfg = ra.DetectorConfig()
    det, agg, _ = detect_sets(ctx, bank, golden_streams[[1, 1]], [[0, 1], [1, 0]], cfg, want_agg=True)
    assert (agg[0, 0] >= agg[0, 1]).all() and agg[0, 0].max() < 0.9999
    assert det[0] and [d[:5] for d in det[0]] == [d[:5] for d in det[1]] and all(d[5] == 1 for v in det for d in v)
    alone, _, _ = detect_sets(ctx, bank, golden_streams[[1]], [[0, -1]], cfg)
    assert not alone[0]


def test_detect_only_full_scores_and_vad(ra, golden_streams):
    """7. Plain detect-only, agg requested and a RP_CTX_FULL_SCORES context give the same detections; the same with VADMode::Easy."""
    full = ra.BatchContext(device=0, host_pointers=True, full_scores=True)
    plain = ra.BatchContext(device=0, host_pointers=True)
    sets = [[0, 1], [1, 2], [2, 0], [1, -1], [2, 1], [0, 1]]
    for vad in (None, ra.VADMode.Easy):
        cfg = ra.DetectorConfig()
        if vad is not None:
            cfg.vad_mode = vad
        got = []
        for c, want in ((plain, False), (plain, True), (full, False)):
            bank = ra.WakewordBank(c, rpw=[read(n) for n in GOLDEN_RPW])
            got.append(detect_sets(c, bank, golden_streams, sets, cfg, want_agg=want)[0])
        assert got[0] == got[1] == got[2] and sum(len(v) for v in got[0]) >= 3, got


# ---------------------------------------------------------------------------------------------- 8. band 0, device pointers, refusals

def test_band_zero_empty_bank_and_empty_rows(ra, ctx, golden, golden_streams):
    """8. band_size 0, an empty bank and rows of all -1: the calls succeed, write zero rows and report nothing."""
    bank, _ = golden
    zero = ra.DetectorConfig()
    zero.band_size = 0
    empty = ra.WakewordBank(ctx, wakewords=[])
    x = golden_streams[:2]
    for bk, cf, sets in ((bank, zero, [[0, 1], [2, -1]]), (empty, ra.DetectorConfig(), [[-1, -1], [-1, -1]]), (bank, ra.DetectorConfig(), [[-1, -1], [-1, -1]])):
        det, agg, avg = detect_sets(ctx, bk, x, sets, cf, want_agg=True)
        assert not any(det) and not agg.any() and not avg.any()
        mf = ctx.mfcc(x, 5)
        nobody = bk is empty or sets[0][0] < 0   # no stream has a window: any pitch will do
        a, g = ctx.dtw_scores_bank_sets(mf, bk, sets, band_size=cf.band_size, with_avg=True, win_pitch=7 if nobody else None)
        assert a.shape[2] > 0 and not a.any() and not g.any()


def test_device_pointer_context(ra, golden_streams, ctx, golden):
    """9. A context without RP_CTX_HOST_POINTERS: everything on the device; an index outside the bank is treated as -1."""
    import torch
    bank_h, _ = golden
    S, max_det = 4, 4
    x = golden_streams[[0, 1, 2, 1]]
    sets = [[0, 1], [1, 7], [-5, 2], [3, -1]]          # 7, -5 and 3 lie outside the bank
    clean = [[0, 1], [1, -1], [-1, 2], [-1, -1]]
    want, w_agg, w_avg = detect_sets(ctx, bank_h, x, clean, ra.DetectorConfig(), want_agg=True)
    dctx = ra.BatchContext(device=0, host_pointers=False)
    bank = ra.WakewordBank(dctx, rpw=[read(n) for n in GOLDEN_RPW])
    nf = ra.api.mfcc_num_frames(x.shape[1])
    pitch = nf - min(bank.max_lens) + 1
    d_pcm = torch.from_numpy(x).cuda()
    d_idx = torch.tensor(sets, dtype=torch.int32, device="cuda")
    d_det = torch.zeros(S * max_det * 24, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(S, dtype=torch.int32, device="cuda")
    d_ww = torch.zeros(S * max_det, dtype=torch.int32, device="cuda")
    d_agg = torch.full((S, 2, pitch), 7.0, dtype=torch.float32, device="cuda")
    d_avg = torch.full((S, 2, pitch), 7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(ra.RustpotterError, match="win_pitch"):
        dctx.batch_detect_bank_sets_dev(d_pcm.data_ptr(), 3, S, x.shape[1], x.shape[1], bank, d_idx.data_ptr(), 2, ra.DetectorConfig(), d_det.data_ptr(),
                                        d_ww.data_ptr(), d_n.data_ptr(), max_det, d_agg.data_ptr(), d_avg.data_ptr(), pitch - 1)
    dctx.batch_detect_bank_sets_dev(d_pcm.data_ptr(), 3, S, x.shape[1], x.shape[1], bank, d_idx.data_ptr(), 2, ra.DetectorConfig(), d_det.data_ptr(),
                                    d_ww.data_ptr(), d_n.data_ptr(), max_det, d_agg.data_ptr(), d_avg.data_ptr(), pitch)
    dctx.synchronize()
    det = np.frombuffer(d_det.cpu().numpy().tobytes(), dtype=ra.api.DET_DTYPE).reshape(S, max_det)
    nd, ww = d_n.cpu().numpy(), d_ww.cpu().numpy().reshape(S, max_det)
    got = [[(int(d["frame"]), int(d["window"]), int(d["counter"]), bits1(d["score"]), bits1(d["avg_score"]), int(ww[s][i]))
            for i, d in enumerate(det[s][:nd[s]])] for s in range(S)]
    assert got == want and any(got) and not got[3]
    a = d_agg.cpu().numpy()
    assert np.array_equal(bits(a[:, :, :w_agg.shape[2]]), bits(w_agg)) and not a[:, :, w_agg.shape[2]:].any()
    assert dctx.dtw_ref_pairs() == 0


def test_refusals(ra, ctx, golden, golden_streams):
    """10. What the header says is refused, each with its message."""
    bank, _ = golden
    L = ra.load_library()
    cfg = ra.DetectorConfig()
    c = cfg._c()
    x = np.ascontiguousarray(golden_streams[:2])
    mf = ctx.mfcc(x, 5)
    nf = mf.shape[1]
    idx = np.array([[0, 1], [2, -1]], np.int32)
    det = np.zeros((2, 4), dtype=ra.api.DET_DTYPE)
    n_det = np.zeros(2, np.int32)
    agg = np.zeros((2, 9, nf), np.float32)

    def score(bank_h=bank._h, mfcc=mf.ctypes.data, sets=idx.ctypes.data, n=2, out=agg.ctypes.data, pitch=nf, band=5):
        return L.rp_dtw_score_bank_sets(ctx._h, mfcc, 2, nf, bank_h, sets, n, 0.22, band, 1, 0, None, out, pitch)

    def detect(bank_h=bank._h, pcm=x.ctypes.data, sets=idx.ctypes.data, n=2, d=det.ctypes.data, nd=n_det.ctypes.data, cf=C.byref(c), a=None, pitch=0):
        return L.rp_batch_detect_bank_sets(ctx._h, pcm, 3, 2, x.shape[1], x.shape[1], bank_h, sets, n, cf, d, None, nd, 4, a, None, pitch)

    assert score() == 0 and detect() == 0
    for n in (0, 9, -1):
        assert score(n=n) == -1 and b"set_size %d is outside 1 .. 8" % n in L.rp_last_error()
        assert detect(n=n) == -1 and b"set_size %d is outside 1 .. 8" % n in L.rp_last_error()
    assert score(bank_h=None) == -1 and b"null handle" in L.rp_last_error()
    assert detect(bank_h=None) == -1 and b"null handle" in L.rp_last_error()
    for kw in (dict(mfcc=None), dict(sets=None), dict(out=None)):
        assert score(**kw) == -1 and b"null argument" in L.rp_last_error(), kw
    for kw in (dict(pcm=None), dict(sets=None), dict(d=None), dict(nd=None), dict(cf=None)):
        assert detect(**kw) == -1 and b"null argument" in L.rp_last_error(), kw
    largest = nf - 126 + 1   # stream 0 holds [0, 1]: alexa's window; stream 1 [2, -1]: 168
    assert score(pitch=largest - 1) == -1 and b"win_pitch %d is smaller than the largest window count of the call (%d)" % (largest - 1, largest) in L.rp_last_error()
    assert score(pitch=largest) == 0
    assert detect(a=agg.ctypes.data, pitch=largest - 1) == -1 and b"win_pitch" in L.rp_last_error()
    for bad, where in ((3, b"stream 1, slot 0"), (-2, b"stream 1, slot 0")):
        b2 = np.array([[0, 1], [bad, 2]], np.int32)
        assert score(sets=b2.ctypes.data) == -1 and where + b": wakeword index %d is outside the bank (-1 .. 2)" % bad in L.rp_last_error()
        assert detect(sets=b2.ctypes.data) == -1 and where + b": wakeword index %d is outside the bank (-1 .. 2)" % bad in L.rp_last_error()
    assert score(band=8) == -1 and b"is not built" in L.rp_last_error()
    other = ra.BatchContext(device=0, host_pointers=True)
    with pytest.raises(ra.RustpotterError, match="the bank belongs to another context"):
        other.batch_detect_bank_sets(x, bank, idx, cfg)
    assert score() == 0 and detect() == 0, "the refusals left the context usable"
