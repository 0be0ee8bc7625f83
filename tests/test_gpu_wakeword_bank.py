"""Wakeword banks (rp_wakeword_bank_*, rp_dtw_score_bank, rp_batch_detect_bank; dtw_bank_kernel, scan_bank_kernel): stream s carries
its own wakeword bank[w(s)].  Checked against today's only alternative -- one rp_batch_detect / rp_dtw_score_batch call per wakeword over
that wakeword's streams under RP_ARITH_STRICT_F32 -- bit for bit, and against the CPU oracle at the project's parity bar (1e-5)."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import rpw_py
import simstream
from oracle import rp_oracle as orc

pytestmark = pytest.mark.gpu

G = simstream.GOLDEN
SEED = 0x5EED00000000BA2C
GOLDEN_RPW = ["alexa.rpw", "oye_casa_g.rpw", "oye_casa_real.rpw"]   # window lengths 126 / 108 / 168, mfcc_size 5, each with an averaged template


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


def read(name):
    with open(os.path.join(G, name), "rb") as f:
        return f.read()


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30))) if a.size else 0.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Wakeword:
    """one wakeword of a test: its templates as rp_templates and what overrides the config"""

    def __init__(self, ra, ctx, templates, avg, threshold=None, avg_threshold=None):
        self.templates, self.avg, self.threshold, self.avg_threshold = templates, avg, threshold, avg_threshold
        self.t = ra.Templates(ctx, templates, avg)
        self.max_len = max(len(t) for t in templates)

    def config(self, ra, base):
        c = ra.DetectorConfig()
        for k, v in vars(base).items():
            setattr(c, k, v)
        if self.threshold is not None:
            c.threshold = self.threshold
        if self.avg_threshold is not None:
            c.avg_threshold = self.avg_threshold
        return c


def from_rpw_dict(ra, ctx, w):
    return Wakeword(ra, ctx, list(w["samples_features"].values()), w["avg_features"], w["threshold"], w["avg_threshold"])


@pytest.fixture(scope="module")
def golden(ra, ctx):
    wws = [from_rpw_dict(ra, ctx, rpw_py.load_rpw(os.path.join(G, n))) for n in GOLDEN_RPW]
    bank = ra.WakewordBank(ctx, rpw=[read(n) for n in GOLDEN_RPW])
    assert bank.max_lens == [126, 108, 168] and bank.max_len == 168 and bank.W == 3
    return bank, wws


def per_wakeword(ra, ctx, pcm, idx, wws, cfg, max_det):
    """today's path: one batch_detect per wakeword over its streams, strict f32 -> per stream (n_det, det rows, agg row)"""
    out = {}
    with ctx.arithmetic("strict_f32"):
        for w, ww in enumerate(wws):
            mine = [s for s in range(len(idx)) if idx[s] == w]
            if not mine:
                continue
            det, n_det, _, agg = ctx.batch_detect(pcm[mine], ww.t, ww.config(ra, cfg), max_det=max_det, want_scores=True)
            for j, s in enumerate(mine):
                out[s] = (int(n_det[j]), det[j], agg[j])
    return out


def check_against_per_wakeword(ra, ctx, bank, wws, pcm, idx, cfg, max_det=4, want_agg=True):
    idx = np.asarray(idx, np.int32)
    want = per_wakeword(ra, ctx, pcm, idx, wws, cfg, max_det)
    before = ctx.get_arithmetic()
    ctx.dtw_kernels()
    res = ctx.batch_detect_bank(pcm, bank, idx, cfg, max_det=max_det, want_agg=want_agg)
    assert "dtw_bank_kernel" in ctx.dtw_kernels() or all(len(want[s][2]) == 0 for s in want)
    assert ctx.get_arithmetic() == before
    det, n_det = res[0], res[1]
    nf = ra.mfcc_num_frames(pcm.shape[1])
    for s in range(len(idx)):
        if idx[s] < 0:
            assert n_det[s] == 0 and not det[s].tobytes().strip(b"\0"), s
            if want_agg:
                assert not res[2][s].any() and not res[3][s].any(), s
            continue
        wn, wd, wa = want[s]
        assert n_det[s] == wn, (s, n_det[s], wn)
        for i in range(min(wn, max_det)):
            for f in ("frame", "window", "counter"):
                assert det[s][i][f] == wd[i][f], (s, i, f)
            assert det[s][i]["stream"] == s
            assert bits(det[s][i]["score"]) == bits(wd[i]["score"]) and bits(det[s][i]["avg_score"]) == bits(wd[i]["avg_score"]), (s, i)
        assert not det[s][min(wn, max_det):].tobytes().strip(b"\0"), "slots behind a stream's detections are zero"
        if want_agg:
            n_win = max(0, nf - wws[idx[s]].max_len + 1)
            assert len(wa) == n_win
            assert np.array_equal(bits(res[2][s][:n_win]), bits(wa)), (s, "agg differs in %d windows" % int(np.sum(bits(res[2][s][:n_win]) != bits(wa))))
            assert not res[2][s][n_win:].any() and not res[3][s][n_win:].any(), s
    return det, n_det


def recording(name):
    a, sr, ch = rpw_py.read_wav(os.path.join(G, name))
    assert ch == 1
    if a.dtype == np.int16:
        a = simstream.i16_to_f32(a)
    if sr == 48000:   # the noise recordings: every third sample (any noise will do here)
        a, sr = a[::3], 16000
    assert sr == 16000 and a.dtype == np.float32
    return a


@pytest.fixture(scope="module")
def golden_streams():
    z = np.zeros(8000, np.float32)
    recs = [np.concatenate([z, recording(n), z]) for n in ("alexa.wav", "oye_casa_g_1.wav", "noise0.wav")]
    n = max(len(r) for r in recs)
    pcm, idx = [], []
    for r in recs:
        for w in range(3):
            pcm.append(np.concatenate([r, np.zeros(n - len(r), np.float32)]))
            idx.append(w)
    pcm.append(pcm[3].copy())   # the oye_casa recording once more, without a wakeword
    idx.append(-1)
    return np.stack(pcm), idx


@pytest.mark.parametrize("mode", ["agg", "detect_only", "eager_vad"])
def test_golden_bank_equals_one_call_per_wakeword(ra, ctx, golden, golden_streams, mode):
    """1. Every recording against every golden wakeword + one stream without a wakeword: n_det, every detection field and (when requested)
    agg bit for bit what rp_batch_detect gives per wakeword; the reference's own golden detection must be among them."""
    bank, wws = golden
    pcm, idx = golden_streams
    cfg = ra.DetectorConfig()
    if mode == "eager_vad":
        cfg.eager, cfg.min_scores, cfg.vad_mode = True, 1, ra.VADMode.Easy
    det, n_det = check_against_per_wakeword(ra, ctx, bank, wws, pcm, idx, cfg, want_agg=(mode == "agg"))
    print("n_det", list(n_det), "oye casa stream:", det[4][0])
    if mode != "eager_vad":
        # tests/detector.rs:24-37: oye_casa_g_1.wav against oye_casa_g.rpw
        assert n_det[4] >= 1
        assert abs(det[4][0]["score"] - 0.7310586) < 5e-7 and abs(det[4][0]["avg_score"] - 0.6495044) < 5e-7, det[4][0]
    else:
        assert n_det[4] >= 1
    assert n_det[9] == 0 and not n_det[6:9].any(), "no wakeword / noise: no detection"


@pytest.mark.parametrize("chunks", [44, 58, 59])
def test_edges_of_the_tile_and_the_window_count(ra, ctx, golden, chunks):
    """2. 129 frames: 4 / 22 / 0 windows; 171 frames: exactly 64 windows at window length 108; 174 frames: 67, a partial second tile.  A stream's
    result does not depend on its neighbours: S = 1 and permuted indices give the same rows."""
    bank, wws = golden
    N = 480 * chunks
    nf = ra.mfcc_num_frames(N)
    assert nf == 3 * chunks - 3
    if chunks == 44:
        assert bank.n_win(nf, [0, 1, 2]) == [4, 22, 0]
    if chunks == 58:
        assert bank.n_win(nf, [1]) == [64]
    if chunks == 59:
        assert bank.n_win(nf, [1]) == [67]
    S = 6
    pcm = ctx.synth_pcm(SEED, 40, S, N)
    cfg = ra.DetectorConfig()
    cfg.threshold, cfg.avg_threshold, cfg.min_scores = 0.3, 0.1, 1   # synthetic noise scores low: let some windows fire
    idx = [0, 1, 2, 1, -1, 0]
    det, n_det = check_against_per_wakeword(ra, ctx, bank, wws, pcm, idx, cfg)
    _, _, agg, avg = ctx.batch_detect_bank(pcm, bank, np.array(idx, np.int32), cfg, max_det=4, want_agg=True)
    for s in range(S):
        if bank.n_win(nf, [idx[s]])[0] == 0:
            assert n_det[s] == 0 and not agg[s].any() and not avg[s].any()
    # one stream alone
    for s in (0, 1, 2):
        d1, n1, a1, v1 = ctx.batch_detect_bank(pcm[s:s + 1], bank, np.array([idx[s]], np.int32), cfg, max_det=4, want_agg=True, win_pitch=agg.shape[1])
        assert n1[0] == n_det[s] and np.array_equal(bits(a1[0]), bits(agg[s])) and np.array_equal(bits(v1[0]), bits(avg[s]))
        for f in ("frame", "window", "counter", "score", "avg_score"):
            assert np.array_equal(d1[0][f], det[s][f])
    # permuted: stream s keeps its PCM, the wakewords move
    perm = [1, 2, 0, 0, 1, -1]
    check_against_per_wakeword(ra, ctx, bank, wws, pcm, perm, cfg)
    det_o, n_o = ctx.batch_detect_bank(pcm, bank, np.array(idx, np.int32), cfg, max_det=4)   # detect-only gives the same detections
    assert np.array_equal(n_o, n_det) and det_o.tobytes() == det.tobytes()


def synth_bank(ra, ctx, K, seed):
    """wakewords of 1..6 templates, 12..60 frames, unequal inside a wakeword; some with an averaged template, some without"""
    rng = np.random.default_rng(seed)
    wws = []
    for w, T in enumerate([1, 2, 3, 6, 4, 5]):
        lens = [int(x) for x in rng.integers(12, 61, T)]
        if T > 1 and len(set(lens)) == 1:
            lens[0] = lens[0] - 1 if lens[0] > 12 else lens[0] + 1
        tm = [orc.synth_templates(SEED + 1000 * K + 50 * w + t, 1, L, K)[0] for t, L in enumerate(lens)]
        avg = None
        if T > 1 and w % 2 == 1:
            avg = orc.average_templates({"t%02d" % t: x for t, x in enumerate(tm)})   # the longest is the origin: never longer than the window
        wws.append(Wakeword(ra, ctx, tm, avg))
    bank = ra.WakewordBank(ctx, wakewords=[(w.templates, w.avg, None, None) for w in wws])
    return bank, wws


def oracle_frames(S, n_frames, K, first):
    n = 480 * (n_frames // 3 + 2)
    return np.stack([orc.mfcc_stream(orc.synth_pcm(SEED, first + s, n), K)[:n_frames] for s in range(S)])


@pytest.mark.parametrize("K,band", [(5, 5), (5, 3), (13, 5), (16, 6)])
def test_scoring_layer_against_the_oracle(ra, ctx, K, band):
    """3. rp_dtw_score_bank on oracle MFCCs: agg / avg within 1e-5 of the oracle per stream with its own wakeword, and bit-equal to
    rp_dtw_score_batch under strict f32 with that wakeword's rp_templates; max, average, median and p90."""
    bank, wws = synth_bank(ra, ctx, K, 7 * K + band)
    S, nf = 8, 90
    mf = oracle_frames(S, nf, K, 500)
    idx = np.array([0, 1, 2, 3, 4, 5, -1, 3], np.int32)
    modes = [("max", ra.ScoreMode.Max), ("average", ra.ScoreMode.Average), ("median", ra.ScoreMode.Median), ("p90", ra.ScoreMode.P90)]
    worst = 0.0
    for name, mode in modes:
        ctx.dtw_kernels()
        avg, agg = ctx.dtw_scores_bank(mf, bank, idx, band_size=band, score_mode=mode, with_avg=True)
        assert ctx.dtw_kernels() == ["dtw_bank_kernel"]
        for s in range(S):
            if idx[s] < 0:
                assert not agg[s].any() and not avg[s].any()
                continue
            ww = wws[idx[s]]
            n_win = nf - ww.max_len + 1
            _, ref_a = orc.score_stream(mf[s], ww.templates, band=band, mode=name)
            worst = max(worst, rel_err(agg[s][:n_win], ref_a))
            assert rel_err(agg[s][:n_win], ref_a) <= 1e-5, (name, s)
            assert not agg[s][n_win:].any() and not avg[s][n_win:].any()
            with ctx.arithmetic("strict_f32"):
                _, b_avg, b_agg = ctx.dtw_scores(mf[s], ww.t, band_size=band, score_mode=mode, with_avg=ww.avg is not None)
            assert np.array_equal(bits(agg[s][:n_win]), bits(b_agg[0])), (name, s)
            if ww.avg is not None:
                ref_v = [orc.score_window(mf[s][w:w + ww.max_len], ww.avg, band=band) for w in range(n_win)]
                assert rel_err(avg[s][:n_win], ref_v) <= 1e-5, (name, s)
                assert np.array_equal(bits(avg[s][:n_win]), bits(b_avg[0])), (name, s)
            else:
                assert not avg[s].any()
    print("K %d band %d: worst relative error against the oracle %.3g" % (K, band, worst))


@pytest.mark.parametrize("K,band", [(7, 5), (5, 8)])
def test_shapes_the_kernel_is_not_built_for_are_refused(ra, ctx, K, band):
    """3b. include/rustpotter_hip.h: mfcc_size 5 / 13 / 16 with band_size 3..6 (or 0); anything else is an error that names the limit."""
    tm = orc.synth_templates(SEED + K, 2, 20, K)
    bank = ra.WakewordBank(ctx, wakewords=[(tm, None, None, None)])
    mf = oracle_frames(1, 40, K, 900)
    with pytest.raises(ra.RustpotterError, match="mfcc_size 5, 13 or 16 with band_size 3..6"):
        ctx.dtw_scores_bank(mf, bank, [0], band_size=band)
    avg, agg = ctx.dtw_scores_bank(mf, bank, [0], band_size=0, with_avg=True)   # band 0: every score 0, as everywhere
    assert agg.shape == (1, 21) and not agg.any() and not avg.any()


def test_norm_range(ra, ctx):
    """4. Frames scaled by 1e-20 / 1e17 and a wakeword whose rows are scaled by 3e-23 (tests/test_gpu_cosine_range.py): the reference-shaped
    cell scores them -- within 1e-5 of the oracle, equal to rp_dtw_score_batch on the same data, and counted."""
    K, nf = 5, 70
    rng = np.random.default_rng(5)
    base = [orc.synth_templates(SEED + 77 + w, 1, L, K)[0] for w, L in enumerate((30, 41, 37))]
    t0 = [base[0], base[1]]
    t1 = [(base[2].astype(np.float64) * 3e-23).astype(np.float32), (base[1].astype(np.float64) * 3e-23).astype(np.float32)]
    wws = [Wakeword(ra, ctx, t0, None), Wakeword(ra, ctx, t1, None)]
    bank = ra.WakewordBank(ctx, wakewords=[(w.templates, None, None, None) for w in wws])
    mf = oracle_frames(4, nf, K, 700)
    mf[1] = (mf[1].astype(np.float64) * 1e-20).astype(np.float32)
    mf[2] = (mf[2].astype(np.float64) * 1e17).astype(np.float32)
    idx = np.array([0, 0, 0, 1], np.int32)
    before = ctx.dtw_ref_pairs()
    _, agg = ctx.dtw_scores_bank(mf, bank, idx)
    assert ctx.dtw_ref_pairs() > before
    for s in range(4):
        ww = wws[idx[s]]
        n_win = nf - ww.max_len + 1
        _, ref_a = orc.score_stream(mf[s], ww.templates)
        assert rel_err(agg[s][:n_win], ref_a) <= 1e-5, s
        with ctx.arithmetic("strict_f32"):
            _, _, b_agg = ctx.dtw_scores(mf[s], ww.t)
        assert np.array_equal(bits(agg[s][:n_win]), bits(b_agg[0])), s
    before = ctx.dtw_ref_pairs()
    ctx.dtw_scores_bank(mf[:1], bank, idx[:1])   # ordinary data: nothing takes the slow path
    assert ctx.dtw_ref_pairs() == before


def wav_bytes(x, rate=16000):
    data = np.clip(np.round(x * 32767), -32768, 32767).astype("<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, 1, rate, rate * 2, 2, 16)
    return b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + \
        b"data" + struct.pack("<I", len(data)) + data


def synth_utterance(rng, seconds):
    """a chirp-like tone under a raised-cosine envelope plus a little noise (the generator idea of tests/test_gpu_enrol_batch.py)"""
    n = int(seconds * 16000)
    t = np.arange(n) / 16000.0
    f0, f1 = rng.uniform(150, 900), rng.uniform(150, 900)
    x = 0.3 * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / t[-1]) + rng.uniform(0, 6)) * np.sin(np.pi * t / t[-1]) ** 2
    return (x + 0.02 * rng.standard_normal(n)).astype(np.float32)


def test_enrol_bank_detect(ra, ctx, tmp_path):
    """5. Enrol (rp_wakeword_ref_build_batch) -> bank (rp_wakeword_bank_new_from_rpw) -> detect: 12 synthetic wakewords of 1..6 samples at
    mfcc_size 13, stream i = sample 0 of wakeword i between silence; detections and agg as one rp_batch_detect per wakeword."""
    rng = np.random.default_rng(12)
    counts = [1, 2, 3, 4, 5, 6, 2, 3, 1, 4, 2, 3]
    wakewords, first = [], []
    for w, n in enumerate(counts):
        base = synth_utterance(rng, rng.uniform(0.5, 0.9))
        samples = {}
        for i in range(n):   # the same utterance, a little longer or shorter and with its own noise
            m = len(base) + int(rng.integers(-800, 801))
            x = np.interp(np.linspace(0, len(base) - 1, m), np.arange(len(base)), base).astype(np.float32)
            x = x + 0.01 * rng.standard_normal(m).astype(np.float32)
            samples["w%02d_%d.wav" % (w, i)] = wav_bytes(x)
            if i == 0:
                first.append(np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16))
        wakewords.append(("ww%02d" % w, samples, 0.45 if w % 3 == 0 else None, 0.1 if w % 4 == 1 else None))
    rpws = ctx.build_wakeword_refs(wakewords, 13)
    bank = ra.WakewordBank(ctx, rpw=rpws)
    wws = []
    for w, b in enumerate(rpws):
        p = tmp_path / ("w%d.rpw" % w)
        p.write_bytes(b)
        d = rpw_py.load_rpw(str(p))
        assert (d["avg_features"] is None) == (counts[w] == 1)
        wws.append(from_rpw_dict(ra, ctx, d))
    assert bank.max_lens == [w.max_len for w in wws]
    z = np.zeros(8000, np.int16)
    n = max(len(x) for x in first) + 16000
    pcm = np.stack([np.concatenate([z, x, np.zeros(n - 8000 - len(x), np.int16)]) for x in first])
    idx = list(range(12))
    det, n_det = check_against_per_wakeword(ra, ctx, bank, wws, pcm, idx, ra.DetectorConfig())
    print("enrol -> bank -> detect: n_det", list(n_det))
    assert n_det.sum() >= 1, "at least one stream must find its own sample"
    assert any(w.avg is None for w in wws)


def test_arguments(ra, ctx, golden, golden_streams):
    """6. Empty calls succeed; bad indices, a short win_pitch, models, mixed mfcc sizes and too many templates are refused; a bank call leaves
    the context's arithmetic and the next rp_batch_detect as they were."""
    bank, wws = golden
    pcm, idx = golden_streams
    cfg = ra.DetectorConfig()
    L = ra.load_library()
    det, n_det = ctx.batch_detect_bank(np.zeros((0, 4800), np.float32), bank, np.zeros(0, np.int32), cfg)
    assert det.shape[0] == 0 and n_det.shape == (0,)
    det, n_det, agg, avg = ctx.batch_detect_bank(pcm[:3], bank, [-1, -1, -1], cfg, want_agg=True, win_pitch=5)
    assert not n_det.any() and not agg.any() and not avg.any() and not det.tobytes().strip(b"\0")
    for bad in (3, -2):
        with pytest.raises(ra.RustpotterError, match="wakeword index %d is outside the bank" % bad):
            ctx.batch_detect_bank(pcm[:2], bank, [0, bad], cfg)
        d, n = np.zeros((2, 4), ra.api.DET_DTYPE), np.zeros(2, np.int32)
        i2 = np.array([0, bad], np.int32)
        c = cfg._c()
        assert L.rp_batch_detect_bank(ctx._h, pcm[:2].ctypes.data, 3, 2, pcm.shape[1], pcm.shape[1], bank._h, i2.ctypes.data, C.byref(c), d.ctypes.data,
                                      n.ctypes.data, 4, None, None, 0) == -1 and b"outside the bank" in L.rp_last_error()
    with pytest.raises(ra.RustpotterError, match="win_pitch 10 is smaller than the largest window count"):
        ctx.batch_detect_bank(pcm[:2], bank, [0, 1], cfg, want_agg=True, win_pitch=10)
    mf = oracle_frames(1, 130, 5, 30)
    with pytest.raises(ra.RustpotterError, match="win_pitch 4 is smaller"):
        ctx.dtw_scores_bank(mf, bank, [0], win_pitch=4)
    assert L.rp_wakeword_bank_max_len(bank._h, 3) == -1 and L.rp_wakeword_bank_max_len(None, 0) == -1
    with pytest.raises(ra.RustpotterError, match=r"^wakeword 1: .*model"):
        ra.WakewordBank(ctx, rpw=[read("alexa.rpw"), read("ok_casa-tiny.rpw")])
    other = ctx.build_wakeword_refs([("x", {"alexa.wav": read("alexa.wav")}, None, None)], 13)[0]
    with pytest.raises(ra.RustpotterError, match=r"^wakeword 2: Usage of wakewords with different mfcc size is not supported"):
        ra.WakewordBank(ctx, rpw=[read("alexa.rpw"), read("oye_casa_g.rpw"), other])
    tm = orc.synth_templates(SEED + 3, 1, 12, 5)
    ra.WakewordBank(ctx, wakewords=[(tm * 32, None, None, None)])   # the cap itself is fine
    with pytest.raises(ra.RustpotterError, match=r"^wakeword 1: 33 templates; a bank takes at most 32"):
        ra.WakewordBank(ctx, wakewords=[(tm, None, None, None), (tm * 33, None, None, None)])
    # the default arithmetic and its results are untouched by a bank call in between
    assert ctx.get_arithmetic()[0] == "f32_matrix"
    d0, n0, s0, a0 = ctx.batch_detect(pcm[3:6], wws[1].t, cfg, want_scores=True)
    ctx.batch_detect_bank(pcm, bank, idx, cfg)
    assert ctx.get_arithmetic()[0] == "f32_matrix"
    d1, n1, s1, a1 = ctx.batch_detect(pcm[3:6], wws[1].t, cfg, want_scores=True)
    assert np.array_equal(n0, n1) and d0.tobytes() == d1.tobytes() and np.array_equal(bits(s0), bits(s1)) and np.array_equal(bits(a0), bits(a1))
