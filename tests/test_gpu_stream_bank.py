"""Live-stream batches over a wakeword bank (rp_stream_batch_new_bank / rp_stream_batch_set_wakewords; dtw_bank_stream_kernel,
scan_bank_stream_kernel): stream s holds its own wakeword bank[w(s)] and is fed chunk by chunk.  Checked bit for bit against the whole-recording
bank call (rp_batch_detect_bank over the concatenation), against the shared-wakeword live batch under RP_ARITH_STRICT_F32 when every stream
indexes the same wakeword, and against the CPU oracle's detector at the project's parity bar (1e-5).  "Bit for bit" holds wherever neither
side rescored a pair with the reference-shaped cosine: the tests assert that none was (ctx.dtw_ref_pairs() does not move)."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import pytest

import rpw_py
import simstream
from oracle import rp_oracle as orc

pytestmark = pytest.mark.gpu

G = simstream.GOLDEN
SEED = 0x5EED0000005B4A2C
GOLDEN_RPW = ["alexa.rpw", "oye_casa_g.rpw", "oye_casa_real.rpw"]   # window lengths 126 / 108 / 168, mfcc_size 5, each with an averaged template
BANK_STREAM = "dtw_bank_stream_kernel"


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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits1(x):
    return int(np.float32(x).view(np.uint32))


def mode_name(m):
    return {0: "average", 1: "max", 2: "median"}[int(m)]


def recording(name):
    """a golden recording as 16 kHz f32 (the 48 kHz ones through the oracle's resampler)"""
    a, sr, ch = rpw_py.read_wav(os.path.join(G, name))
    assert ch == 1
    if a.dtype == np.int16:
        a = simstream.i16_to_f32(a)
    if sr != 16000:
        a = orc.resample_stream(a, sr)
    return np.ascontiguousarray(a, np.float32)


def quiet(rng, n):
    """'silence' that is not digital zero: a window of identical frames would sit on the edge of the fast cosine's norm range"""
    return (1e-3 * rng.standard_normal(n)).astype(np.float32)


def feed(sb, pcm, pieces, max_det=8, want_agg=False, before_chunk=None):
    """pcm [S][C * samples_per_chunk] through the batch in calls of pieces[0], pieces[1], ... chunks (cycled; the last call takes what is
    left).  -> per stream the list of (frame, window, counter, score bits, avg_score bits, wakeword, label), and agg [S][frames] or None.
    before_chunk(c): called between calls, before the chunk with index c is fed.  (A stream emits at most one detection per chunk: max_det 8
    holds every call of up to eight chunks.)"""
    spc, fpc = sb.samples_per_chunk, sb.frames_per_chunk
    S, total = pcm.shape[0], pcm.shape[1] // spc
    assert total * spc == pcm.shape[1]
    out, aggs = [[] for _ in range(S)], []
    c = k = 0
    while c < total:
        n = min(pieces[k % len(pieces)], total - c)
        k += 1
        if before_chunk is not None:
            before_chunk(c)
        part = np.ascontiguousarray(pcm[:, c * spc:(c + n) * spc])
        if want_agg:
            det, n_det, agg = sb.process(part, max_det=max_det, want_agg=True)
            assert agg.shape == (S, fpc * n)
            aggs.append(agg)
            dww = dlab = None
        else:
            det, dww, dlab, n_det = sb.process_multi(part, max_det=max_det)
        for s in range(S):
            assert n_det[s] <= max_det
            for i in range(n_det[s]):
                d = det[s][i]
                assert d["stream"] == s
                out[s].append((int(d["frame"]), int(d["window"]), int(d["counter"]), bits1(d["score"]), bits1(d["avg_score"]),
                               None if dww is None else int(dww[s][i]), None if dlab is None else int(dlab[s][i])))
            assert not det[s][n_det[s]:].tobytes().strip(b"\0"), "slots behind a stream's detections are zero"
        c += n
    return out, (np.concatenate(aggs, axis=1) if want_agg else None)


def whole(ctx, bank, pcm, idx, cfg, max_det=32, want_agg=False):
    """rp_batch_detect_bank over the concatenation -> per stream the list of (frame, window, counter, score bits, avg bits), agg, avg"""
    res = ctx.batch_detect_bank(pcm, bank, np.asarray(idx, np.int32), cfg, max_det=max_det, want_agg=want_agg)
    det, n_det = res[0], res[1]
    out = []
    for s in range(len(idx)):
        assert n_det[s] <= max_det
        out.append([(int(d["frame"]), int(d["window"]), int(d["counter"]), bits1(d["score"]), bits1(d["avg_score"])) for d in det[s][:n_det[s]]])
    return (out, res[2], res[3]) if want_agg else (out, None, None)


def same_detections(live, ref, idx=None):
    for s in range(len(ref)):
        assert [d[:5] for d in live[s]] == ref[s], (s, live[s], ref[s])
        if idx is not None:
            assert all(d[5] in (None, idx[s]) and d[6] in (None, -1) for d in live[s]), (s, live[s])


def same_aggregates(bank, idx, live_agg, whole_agg, fpc=3):
    """the live aggregate at frame f >= max_len(s) - 1 is the whole call's agg[s][f - max_len(s) + 1]; column j of the live rows is frame j - fpc"""
    n = 0
    for s, w in enumerate(idx):
        if w < 0:
            assert not live_agg[s].any(), s
            continue
        L = bank.max_lens[w]
        f = np.arange(L - 1, live_agg.shape[1] - fpc)
        assert len(f) > 0, "the stream is too short for its window"
        a, b = bits(live_agg[s][f + fpc]), bits(whole_agg[s][f - L + 1])
        assert np.array_equal(a, b), (s, w, "agg differs in %d of %d windows" % (int(np.sum(a != b)), len(f)))
        n += len(f)
    return n


# ---------------------------------------------------------------------------------------------- 1. golden bank, live = whole

@pytest.fixture(scope="module")
def golden(ra, ctx):
    dicts = [rpw_py.load_rpw(os.path.join(G, n)) for n in GOLDEN_RPW]
    bank = ra.WakewordBank(ctx, rpw=[read(n) for n in GOLDEN_RPW])
    assert bank.max_lens == [126, 108, 168] and bank.max_len == 168 and bank.W == 3
    return bank, dicts


@pytest.fixture(scope="module")
def golden_streams():
    rng = np.random.default_rng(31)
    recs = {n: recording(n) for n in ("alexa.wav", "oye_casa_g_1.wav", "oye_casa_real_1.wav")}
    recs["noise"] = (0.1 * rng.standard_normal(20000)).astype(np.float32)
    plan = [("alexa.wav", 0), ("alexa.wav", 1), ("oye_casa_g_1.wav", 1), ("oye_casa_g_1.wav", 2), ("oye_casa_g_1.wav", -1),
            ("oye_casa_real_1.wav", 2), ("oye_casa_real_1.wav", 0), ("noise", 0), ("noise", 1)]
    # 0.5 s in front, at least 1.5 s behind (the longest countdown is 84 frames): no detection is pending at the end
    n = 480 * ((8000 + max(len(r) for r in recs.values()) + 24000 + 479) // 480)
    pcm = np.stack([np.concatenate([quiet(rng, 8000), recs[name], quiet(rng, n - 8000 - len(recs[name]))]) for name, _ in plan])
    return pcm, [w for _, w in plan]


@pytest.fixture(scope="module")
def golden_whole(ra, ctx, golden, golden_streams):
    bank, _ = golden
    pcm, idx = golden_streams
    before = ctx.dtw_ref_pairs()
    ref, _, _ = whole(ctx, bank, pcm, idx, ra.DetectorConfig())
    assert ctx.dtw_ref_pairs() == before
    return ref


def oracle_detections(wdict, pcm, cfg):
    """orc.Detector = Rustpotter::new(config) + add_wakeword(wdict, with its own thresholds) + process_samples per 30 ms chunk"""
    d = orc.Detector(avg_threshold=cfg.avg_threshold, threshold=cfg.threshold, min_scores=cfg.min_scores, eager=cfg.eager,
                     score_ref=cfg.score_ref, band_size=cfg.band_size, score_mode=mode_name(cfg.score_mode))
    d.add_ref(wdict)
    return [(i // 480, r) for i in range(0, len(pcm) - 479, 480) for r in [d.process_f32(pcm[i:i + 480])] if r is not None]


@pytest.fixture(scope="module")
def golden_oracle(ra, golden, golden_streams):
    _, dicts = golden
    pcm, idx = golden_streams
    return [oracle_detections(dicts[w], pcm[s], ra.DetectorConfig()) if w >= 0 else [] for s, w in enumerate(idx)]


@pytest.mark.parametrize("pieces", [(1,), (8,), (3, 1, 2)])
def test_golden_bank_live_equals_whole(ra, ctx, golden, golden_streams, golden_whole, golden_oracle, pieces):
    """1. Nine streams (three golden recordings and noise between quiet stretches, indices mixed, one stream without a wakeword) fed in
    pieces: every stream's detections are those of rp_batch_detect_bank over the concatenation -- n_det, frame, window, counter, score and
    avg_score bits -- with det_wakeword the stream's index and label -1; every golden wakeword fires at least once; and the detections
    agree with the oracle's detector fed the same chunks at 1e-5, chunk and counter exact."""
    bank, _ = golden
    pcm, idx = golden_streams
    cfg = ra.DetectorConfig()
    before, arith = ctx.dtw_ref_pairs(), ctx.get_arithmetic()
    ctx.dtw_kernels()
    sb = ra.StreamBatch(ctx, None, cfg, len(idx), max_chunks_per_call=8, bank=bank, stream_wakeword=idx)
    live, _ = feed(sb, pcm, pieces)
    assert BANK_STREAM in ctx.dtw_kernels() and ctx.get_arithmetic() == arith
    assert ctx.dtw_ref_pairs() == before
    assert sb.chunks_seen == pcm.shape[1] // 480
    same_detections(live, golden_whole, idx)
    print("detections per stream:", [len(d) for d in live])
    for w in range(3):
        assert any(live[s] for s in range(len(idx)) if idx[s] == w), "golden wakeword %d never fired" % w
    assert not live[4] and not live[7] and not live[8], "no wakeword / noise: no detection"
    worst = 0.0
    for s, want in enumerate(golden_oracle):
        assert len(live[s]) == len(want), (s, live[s], want)
        for d, (chunk, r) in zip(live[s], want):
            assert d[0] // 3 + 1 == chunk and d[2] == r["counter"], (s, d, chunk, r)
            sc, av = np.array([d[3]], np.uint32).view(np.float32)[0], np.array([d[4]], np.uint32).view(np.float32)[0]
            e = abs(float(sc) - float(r["score"])) / float(r["score"])
            if r["avg_score"] == 0:
                assert av == 0
            else:
                e = max(e, abs(float(av) - float(r["avg_score"])) / float(r["avg_score"]))
            assert e <= 1e-5, (s, d, r)
            worst = max(worst, e)
    print("worst relative error against the oracle's detector: %.3g" % worst)


# ---------------------------------------------------------------------------------------------- 2. aggregates and lane divergence

# (template count, template lengths): 1, 2, 5 and 32 templates, ragged inside a wakeword, with the lengths 1, 2, 7, 40, 64 and 65
SHAPES = [(1, [1]), (2, [2, 1]), (1, [7]), (5, [40, 7, 33, 2, 39]), (2, [64, 65]), (32, None), (5, [65, 64, 40, 7, 1]), (2, [40, 40]),
          (1, [64]), (5, [12, 30, 18, 25, 29]), (2, [7, 2])]
_SYNTH = {}


def synth_bank(ra, ctx, K):
    """22 wakewords: SHAPES twice, the second copy of a wakeword with several templates carries an averaged template (and so do the
    32-template ones); window lengths 1 .. 65"""
    if K in _SYNTH:
        return _SYNTH[K]
    rng = np.random.default_rng(100 + K)
    wakewords = []
    for copy in range(2):
        for w, (T, lens) in enumerate(SHAPES):
            if lens is None:
                lens = [int(x) for x in rng.integers(20, 50, T)]
            tm = [orc.synth_templates(SEED + 100000 * K + 1000 * copy + 50 * w + t, 1, L, K)[0] for t, L in enumerate(lens)]
            avg = None
            if T > 1 and (copy == 1 or T == 32):
                avg = orc.average_templates(OrderedDict(("t%02d" % t, x) for t, x in enumerate(tm)))
                assert len(avg) <= max(lens)
            wakewords.append((tm, avg, None, None))
    bank = ra.WakewordBank(ctx, wakewords=wakewords)
    assert bank.W == 22 and bank.max_len == 65 and min(bank.max_lens) == 1
    _SYNTH[K] = (bank, wakewords)
    return _SYNTH[K]


CHUNKS = 32   # 93 frames: every window length of the synthetic banks has windows, the longest 29


@pytest.fixture(scope="module")
def noise45(ctx):
    return ctx.synth_pcm(SEED, 7, 45, 480 * CHUNKS)


@pytest.mark.parametrize("mode", ["Max", "Average", "Median"])
@pytest.mark.parametrize("K,band", [(5, 3), (5, 4), (5, 5), (5, 6), (13, 5), (13, 6), (16, 5), (16, 6)])
def test_aggregates_of_ragged_banks(ra, ctx, noise45, K, band, mode):
    """2. 45 streams x one chunk = 135 rows: ~21 different wakewords in a wave (1 .. 32 templates of 1 .. 65 frames, with and without an
    averaged template, three streams without a wakeword), the last wave ragged; one stream alone; five streams x eight chunks.  The live
    aggregate of every window that lies inside the stream is rp_batch_detect_bank's, bit for bit."""
    bank, _ = synth_bank(ra, ctx, K)
    cfg = ra.DetectorConfig()
    cfg.band_size, cfg.score_mode = band, getattr(ra.ScoreMode, mode)
    idx = [s % 22 for s in range(45)]
    idx[5] = idx[30] = idx[44] = -1
    before, arith = ctx.dtw_ref_pairs(), ctx.get_arithmetic()
    _, w_agg, _ = whole(ctx, bank, noise45, idx, cfg, want_agg=True)
    compared = 0
    for streams, per_call in ((range(45), 1), ([13], 1), ([3, 4, 5, 26, 27], 8)):
        streams = list(streams)
        sub = [idx[s] for s in streams]
        ctx.dtw_kernels()
        sb = ra.StreamBatch(ctx, None, cfg, len(streams), max_chunks_per_call=per_call, bank=bank, stream_wakeword=sub)
        _, l_agg = feed(sb, noise45[streams], (per_call,), want_agg=True)
        assert BANK_STREAM in ctx.dtw_kernels() and ctx.get_arithmetic() == arith
        assert l_agg.shape == (len(streams), 3 * CHUNKS)
        compared += same_aggregates(bank, sub, l_agg, w_agg[streams])
    assert ctx.dtw_ref_pairs() == before
    print("K %d band %d %s: %d windows bit-equal" % (K, band, mode, compared))


# ---------------------------------------------------------------------------------------------- 3. gate and per-wakeword thresholds

def test_gate_and_own_thresholds(ra, ctx, noise45):
    """3. Detect-only calls (no agg: a window below its avg_threshold is not compared with the sample templates) report the detections of
    fully scored calls, with an avg_threshold that puts lanes of one wave on both sides (shown from the fully scored avg values); and a
    wakeword's own threshold / avg_threshold override the config's."""
    K = 5
    _, wakewords = synth_bank(ra, ctx, K)
    cfg = ra.DetectorConfig()
    cfg.min_scores = 1
    S = 45
    with_avg = [w for w in range(22) if wakewords[w][1] is not None]
    idx = [with_avg[s % len(with_avg)] for s in range(S)]
    bank0 = ra.WakewordBank(ctx, wakewords=wakewords)
    cfg.avg_threshold, cfg.threshold = 1e-6, 2.0   # every window's averaged template is scored, nothing fires
    _, agg, avg = whole(ctx, bank0, noise45, idx, cfg, want_agg=True)
    nf = 3 * CHUNKS - 3
    valid = [np.arange(nf - bank0.max_lens[w] + 1) for w in idx]
    cfg.avg_threshold = float(np.median(np.concatenate([avg[s][v] for s, v in enumerate(valid)])))
    cfg.threshold = float(np.quantile(np.concatenate([agg[s][v] for s, v in enumerate(valid)]), 0.6))
    # wave 0 of the call that brings frames 87..89: rows (s, i), s = 0..20; lanes on both sides of the gate
    f = 88
    lanes = np.array([avg[s][f - bank0.max_lens[idx[s]] + 1] for s in range(21)])
    assert (lanes < cfg.avg_threshold).any() and (lanes >= cfg.avg_threshold).any(), lanes
    before = ctx.dtw_ref_pairs()
    # two wakewords get values of their own: the one that fires most under the config's a threshold that can never be passed, another an
    # avg_threshold that everything passes
    ref0, _, _ = whole(ctx, bank0, noise45, idx, cfg)
    fired = {w: sum(len(ref0[s]) for s in range(S) if idx[s] == w) for w in with_avg}
    a = max(fired, key=fired.get)
    b = [w for w in with_avg if w != a][0]
    assert fired[a] > 0, "the thresholds were chosen so that windows fire"
    own = list(wakewords)
    own[a] = (wakewords[a][0], wakewords[a][1], 0.9999, None)
    own[b] = (wakewords[b][0], wakewords[b][1], None, 1e-6)
    bank = ra.WakewordBank(ctx, wakewords=own)
    ref, _, _ = whole(ctx, bank, noise45, idx, cfg, want_agg=True)
    gated = ra.StreamBatch(ctx, None, cfg, S, bank=bank, stream_wakeword=idx)
    full = ra.StreamBatch(ctx, None, cfg, S, bank=bank, stream_wakeword=idx)
    live_g, _ = feed(gated, noise45, (1,))
    live_f, _ = feed(full, noise45, (1,), want_agg=True)
    assert ctx.dtw_ref_pairs() == before
    same_detections(live_g, ref, idx)
    same_detections(live_f, ref)
    n = [len(d) for d in live_g]
    print("detections per stream:", n)
    assert sum(n) > 0, "the thresholds were chosen so that windows fire"
    assert all(not live_g[s] for s in range(S) if idx[s] == a), "own threshold 0.9999: never fires"
    # streams of the other wakewords are what they were without own values
    for s in range(S):
        if idx[s] not in (a, b):
            assert ref[s] == ref0[s], s


# ---------------------------------------------------------------------------------------------- 4. uniform bank == shared-wakeword batch

def resampled(x, rate):
    """the 16 kHz stream x as it would sound at `rate` (linear interpolation: any audio will do, both batches get the same)"""
    n = int(len(x) * rate / 16000)
    return np.interp(np.arange(n) * (16000.0 / rate), np.arange(len(x)), x).astype(np.float32)


@pytest.mark.parametrize("case", ["16k", "48k", "22k", "band_pass"])
def test_uniform_bank_equals_shared_wakeword_batch(ra, ctx, golden, golden_streams, case):
    """4. Every stream indexes oye_casa_g: detections and aggregates equal, bit for bit, those of rp_stream_batch_new with that wakeword's
    rp_templates under RP_ARITH_STRICT_F32 -- plain 16 kHz, 48 kHz through set_input, 22.05 kHz with its 40 ms frames (four frames a
    chunk), and the band-pass filter alone with levels(); VAD on."""
    bank, dicts = golden
    pcm16, _ = golden_streams
    w = 1
    d = dicts[w]
    tm = ra.Templates(ctx, list(d["samples_features"].values()), d["avg_features"])
    cfg = ra.DetectorConfig()
    cfg.vad_mode = ra.VADMode.Easy
    shared_cfg = ra.DetectorConfig()
    for k, v in vars(cfg).items():
        setattr(shared_cfg, k, v)
    if d["threshold"] is not None:
        shared_cfg.threshold = d["threshold"]
    if d["avg_threshold"] is not None:
        shared_cfg.avg_threshold = d["avg_threshold"]
    streams = [2, 0, 7]   # oye_casa_g_1, alexa, noise
    rate = {"16k": 16000, "48k": 48000, "22k": 22050, "band_pass": 16000}[case]
    kw = {}
    if case == "band_pass":
        f = ra.FiltersConfig()
        f.band_pass.enabled, f.band_pass.low_cutoff, f.band_pass.high_cutoff = True, 80.0, 2000.0
        kw = dict(filters=f)
    a = ra.StreamBatch(ctx, None, cfg, 3, max_chunks_per_call=4, sample_rate=rate, bank=bank, stream_wakeword=[w, w, w], **kw)
    b = ra.StreamBatch(ctx, tm, shared_cfg, 3, max_chunks_per_call=4, sample_rate=rate, **kw)
    spc = a.samples_per_chunk
    assert spc == b.samples_per_chunk and a.frames_per_chunk == (4 if case == "22k" else 3)
    x = [pcm16[s] if rate == 16000 else resampled(pcm16[s], rate) for s in streams]
    n = spc * (min(len(v) for v in x) // spc)
    pcm = np.stack([v[:n] for v in x])
    before = ctx.dtw_ref_pairs()
    levels = []
    live_a, agg_a = feed(a, pcm, (4, 1), want_agg=True, before_chunk=lambda c: levels.append(a.levels()) if c and case == "band_pass" else None)
    with ctx.arithmetic("strict_f32"):
        k = [0]

        def check_levels(c):
            if c and case == "band_pass":
                r, g = b.levels()
                assert np.array_equal(bits(r), bits(levels[k[0]][0])) and np.array_equal(bits(g), bits(levels[k[0]][1])), c
                k[0] += 1
        live_b, agg_b = feed(b, pcm, (4, 1), want_agg=True, before_chunk=check_levels)
    assert ctx.dtw_ref_pairs() == before
    assert live_a == live_b, (live_a, live_b)
    fpc = a.frames_per_chunk
    col = np.arange(fpc + bank.max_lens[w] - 1, agg_a.shape[1])   # windows that lie inside the stream
    assert np.array_equal(bits(agg_a[:, col]), bits(agg_b[:, col]))
    if case == "band_pass":
        assert k[0] == len(levels) > 0
    if case == "16k":
        assert live_a[0], "the oye casa recording fires"
    print(case, "detections per stream:", [len(v) for v in live_a])


# ---------------------------------------------------------------------------------------------- 5. slots

def test_slots(ra, ctx, golden, golden_streams):
    """5. rp_stream_batch_set_wakewords is connect / disconnect: a stream re-targeted to wakeword j after chunk c reports, from then on,
    exactly what a stream that always had j and got rp_stream_batch_reset after chunk c reports; the other streams never notice; a stream
    set to -1 reports nothing; -1 -> j behaves like i -> j."""
    bank, _ = golden
    pcm, _ = golden_streams
    cfg = ra.DetectorConfig()
    streams = [2, 2, 2, 0, 2]     # oye_casa_g_1 x 3, alexa, oye_casa_g_1
    x = pcm[streams]
    c0 = 10                       # before the utterance (it starts in chunk 16): the window refills in time to see all of it
    before = ctx.dtw_ref_pairs()
    A = ra.StreamBatch(ctx, None, cfg, 5, bank=bank, stream_wakeword=[1, 1, 1, 0, 1])
    B = ra.StreamBatch(ctx, None, cfg, 5, bank=bank, stream_wakeword=[2, -1, 1, 0, 1])

    def act_a(c):
        if c == c0:
            A.reset(0)
            A.reset(1)

    def act_b(c):
        if c == c0:
            B.set_wakewords(0, [1, 1])      # 2 -> 1 and -1 -> 1
            B.set_wakewords(4, [-1])        # disconnect
    live_a, _ = feed(A, x, (1,), before_chunk=act_a)
    live_b, _ = feed(B, x, (1,), before_chunk=act_b)
    assert ctx.dtw_ref_pairs() == before
    frame0 = 3 * c0 - 3
    for s in (0, 1):
        from_c = [d for d in live_a[s] if d[0] >= frame0]
        assert from_c and [d for d in live_b[s] if d[0] >= frame0] == from_c, (s, live_a[s], live_b[s])
    assert not [d for d in live_b[1] if d[0] < frame0], "a stream without a wakeword reports nothing"
    assert live_b[2] == live_a[2] and live_b[3] == live_a[3] and live_a[2] and live_a[3], "the other streams are untouched"
    assert live_a[4] and not [d for d in live_b[4] if d[0] >= frame0], "index -> -1 reports nothing afterwards"


# ---------------------------------------------------------------------------------------------- 6. device pointers

def test_device_pointer_context(ra, golden_streams, golden_whole):
    """6. A context without RP_CTX_HOST_POINTERS: indices, audio and outputs on the device; an index outside the bank is treated as -1;
    the detections are those of the host-pointer run."""
    import torch
    pcm, idx = golden_streams
    S, max_det = len(idx), 4
    dctx = ra.BatchContext(device=0, host_pointers=False)
    bank = ra.WakewordBank(dctx, rpw=[read(n) for n in GOLDEN_RPW])
    cfg = ra.DetectorConfig()
    bad = list(idx)
    bad[4], bad[7] = 3, -7      # outside the bank: stream 4 had -1 anyway, stream 7 (noise) reports nothing either way
    d_idx = torch.tensor(bad, dtype=torch.int32, device="cuda")
    sb = ra.StreamBatch(dctx, None, cfg, S, max_chunks_per_call=8, bank=bank, stream_wakeword=int(d_idx.data_ptr()))
    d_pcm = torch.from_numpy(pcm).cuda()
    d_det = torch.zeros(S * max_det * 24, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(S, dtype=torch.int32, device="cuda")
    d_ww = torch.zeros(S * max_det, dtype=torch.int32, device="cuda")
    d_lab = torch.zeros(S * max_det, dtype=torch.int32, device="cuda")
    got = [[] for _ in range(S)]
    total = pcm.shape[1] // 480
    c = 0
    while c < total:
        n = min(8, total - c)
        part = d_pcm[:, c * 480:(c + n) * 480].contiguous()
        sb.process_multi_dev(part.data_ptr(), 3, n, n * 480, d_det.data_ptr(), d_ww.data_ptr(), d_lab.data_ptr(), d_n.data_ptr(), max_det)
        dctx.synchronize()
        det = np.frombuffer(d_det.cpu().numpy().tobytes(), dtype=ra.api.DET_DTYPE).reshape(S, max_det)
        nd, ww, lab = d_n.cpu().numpy(), d_ww.cpu().numpy().reshape(S, max_det), d_lab.cpu().numpy().reshape(S, max_det)
        for s in range(S):
            for i in range(nd[s]):
                d = det[s][i]
                got[s].append((int(d["frame"]), int(d["window"]), int(d["counter"]), bits1(d["score"]), bits1(d["avg_score"])))
                assert ww[s][i] == idx[s] and lab[s][i] == -1
        c += n
    assert dctx.dtw_ref_pairs() == 0
    assert got == golden_whole and any(got)
    # set_wakewords with a device array
    d_two = torch.tensor([1, 9], dtype=torch.int32, device="cuda")
    sb.set_wakewords(0, int(d_two.data_ptr()), n=2)
    dctx.synchronize()


# ---------------------------------------------------------------------------------------------- 7. refusals

def test_refusals(ra, ctx, golden):
    """7. What the header says is refused, each with its message; an empty bank and band_size 0 succeed and report nothing."""
    bank, dicts = golden
    cfg = ra.DetectorConfig()
    L = ra.load_library()
    c = cfg._c()
    h = C.c_void_p()
    idx = np.array([0, 1], np.int32)
    assert L.rp_stream_batch_new_bank(ctx._h, None, idx.ctypes.data, C.byref(c), 2, 1, C.byref(h)) == -1 and b"null handle" in L.rp_last_error()
    assert L.rp_stream_batch_new_bank(ctx._h, bank._h, None, C.byref(c), 2, 1, C.byref(h)) == -1 and b"null argument" in L.rp_last_error()
    assert L.rp_stream_batch_new_bank(ctx._h, bank._h, idx.ctypes.data, C.byref(c), 0, 1, C.byref(h)) == -1 and b"must be >= 1" in L.rp_last_error()
    other = ra.BatchContext(device=0, host_pointers=True)
    with pytest.raises(ra.RustpotterError, match="the bank belongs to another context"):
        ra.StreamBatch(other, None, cfg, 2, bank=bank, stream_wakeword=[0, 1])
    for bad in (3, -2):
        with pytest.raises(ra.RustpotterError, match=r"^stream 1: wakeword index %d is outside the bank \(-1 .. 2\)" % bad):
            ra.StreamBatch(ctx, None, cfg, 3, bank=bank, stream_wakeword=[0, bad, 1])
    wide = ra.DetectorConfig()
    wide.band_size = 8
    with pytest.raises(ra.RustpotterError, match="wakeword bank: mfcc_size 5 with band_size 8 is not built"):
        ra.StreamBatch(ctx, None, wide, 2, bank=bank, stream_wakeword=[0, 1])
    bank7 = ra.WakewordBank(ctx, wakewords=[(orc.synth_templates(SEED, 2, 20, 7), None, None, None)])
    with pytest.raises(ra.RustpotterError, match="wakeword bank: mfcc_size 7 with band_size 5 is not built"):
        ra.StreamBatch(ctx, None, cfg, 1, bank=bank7, stream_wakeword=[0])
    sb = ra.StreamBatch(ctx, None, cfg, 2, max_chunks_per_call=2, bank=bank, stream_wakeword=[0, 1])
    f = ra.FiltersConfig()
    f.gain_normalizer.enabled = True
    with pytest.raises(ra.RustpotterError, match="gain normaliser is not available on a batch over a wakeword bank"):
        sb.set_filters(f, 0.05)
    with pytest.raises(ra.RustpotterError, match=r"reach past the batch's 2 streams"):
        sb.set_wakewords(1, [0, 1])
    with pytest.raises(ra.RustpotterError, match=r"^stream 1: wakeword index 5 is outside the bank"):
        sb.set_wakewords(0, [1, 5])
    assert L.rp_stream_batch_set_wakewords(sb._h, 0, 1, None) == -1 and b"null argument" in L.rp_last_error()
    sb.set_wakewords(2, [])   # an empty range at the end is fine
    with pytest.raises(ra.RustpotterError, match="n_chunks out of range"):
        sb.process_multi(np.zeros((2, 3 * 480), np.float32))
    det, dww, dlab, n_det = sb.process_multi(np.zeros((2, 2 * 480), np.float32))   # the refusals above left the batch usable
    assert not n_det.any()
    d = dicts[1]
    tm = ra.Templates(ctx, list(d["samples_features"].values()), d["avg_features"])
    shared = ra.StreamBatch(ctx, tm, cfg, 2)
    with pytest.raises(ra.RustpotterError, match="was not made by rp_stream_batch_new_bank"):
        shared.set_wakewords(0, [0])
    # an empty bank, all indices -1, band_size 0: calls succeed, zero rows, no detection
    rng = np.random.default_rng(3)
    noise = (0.1 * rng.standard_normal((2, 480 * 60))).astype(np.float32)
    empty = ra.WakewordBank(ctx, wakewords=[])
    zero = ra.DetectorConfig()
    zero.band_size, zero.threshold = 0, 0.2
    for bk, cf, ix in ((empty, wide, [-1, -1]), (bank, cfg, [-1, -1]), (bank, zero, [0, 1])):
        sb = ra.StreamBatch(ctx, None, cf, 2, max_chunks_per_call=4, bank=bk, stream_wakeword=ix)
        live, agg = feed(sb, noise, (4,), want_agg=True)
        assert not any(live) and not agg.any()
