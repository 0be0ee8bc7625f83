"""RustpotterConfig.filters for live-stream batches (rp_stream_batch_set_filters / rp_stream_batch_levels): the gain normaliser and the
band-pass with their state carried per stream on the device, against the reference's goldens, the oracle's front-end and chunk-wise
detector, and the whole-stream calls (rp_frontend_batch -> rp_batch_detect*) bit for bit."""
import json
import os

import numpy as np
import pytest

import rpw_py
import simstream
from oracle import rp_oracle as orc

pytestmark = pytest.mark.gpu
G = simstream.GOLDEN
EXP = json.load(open(os.path.join(G, "expectations.json")))
SEED = 0x5EED000000000001
PIECES = [(1,), (3, 1, 2), (4,)]


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


def _filters(ra, gain=False, band=False, min_gain=0.1, max_gain=1.0, low=80.0, high=400.0, gain_ref=None):
    f = ra.FiltersConfig()
    f.gain_normalizer.enabled, f.gain_normalizer.min_gain, f.gain_normalizer.max_gain = gain, min_gain, max_gain
    f.gain_normalizer.gain_ref = gain_ref
    f.band_pass.enabled, f.band_pass.low_cutoff, f.band_pass.high_cutoff = band, low, high
    return f


def _golden_config(ra, e):
    c = ra.RustpotterConfig.default()
    c.detector.avg_threshold, c.detector.threshold = e["avg_threshold"], e["threshold"]
    c.detector.min_scores = e.get("min_scores", 5)
    c.detector.score_mode = {"max": ra.ScoreMode.Max, "median": ra.ScoreMode.Median, "average": ra.ScoreMode.Average}[e["score_mode"]]
    c.filters = _filters(ra, e.get("gain_normalizer", False), e.get("band_pass", False), e.get("min_gain", 0.1), e.get("max_gain", 1.0),
                         e.get("low_cutoff", 80.0), e.get("high_cutoff", 400.0))
    return c


def _det_tuple(d):
    return (int(d["frame"]), int(d["window"]), int(d["counter"]), float(d["score"]), float(d["avg_score"]))


def _same(rec, ref):
    return all(rec[f] == ref[f] for f in ("frame", "window", "counter")) and rec["score"].tobytes() == ref["score"].tobytes() and \
        rec["avg_score"].tobytes() == ref["avg_score"].tobytes()


def _feed(sb, pcm, pieces, want_agg=True, levels=True, spc=480, before_call=None):
    """pcm [S][N] through the batch in calls of pieces[i % len] chunks -> (detections per stream, agg [S][frames], rms [S][chunks],
    gains [S][chunks]); before_call(first chunk of the call) runs ahead of every call."""
    S, N = pcm.shape
    got = [[] for _ in range(S)]
    aggs, rms, gains = [], [], []
    pos, k = 0, 0
    while pos < N:
        nc = min(pieces[k % len(pieces)], (N - pos) // spc)
        k += 1
        if before_call is not None:
            before_call(pos // spc)
        r = sb.process(pcm[:, pos:pos + spc * nc], want_agg=want_agg)
        pos += spc * nc
        d, nd = r[0], r[1]
        for s in range(S):
            assert nd[s] <= d.shape[1]
            for j in range(nd[s]):
                assert d[s][j]["stream"] == s
                got[s].append(d[s][j].copy())
        if want_agg:
            aggs.append(r[2].copy())
        if levels:
            lr, lg = sb.levels()
            assert lr.shape == (S, nc) and lg.shape == (S, nc)
            rms.append(lr); gains.append(lg)
    return got, (np.concatenate(aggs, axis=1) if want_agg else None), (np.concatenate(rms, axis=1) if levels else None), \
        (np.concatenate(gains, axis=1) if levels else None)


def _agg_equal_offline(live_agg, agg, L, fpf=3):
    """column k of the live aggregates is the window that ends at frame k - fpf: row k - fpf - L + 1 of the offline aggregates"""
    n = 0
    for k in range(live_agg.shape[1]):
        wi = k - fpf - L + 1
        if 0 <= wi < agg.shape[1]:
            assert np.array_equal(live_agg[:, k].view(np.uint32), agg[:, wi].view(np.uint32)), k
            n += 1
    return n


@pytest.mark.parametrize("pieces", PIECES)
@pytest.mark.parametrize("case,chunks", [("band_pass", (224, 428)), ("gain_normalizer", (224, 429)), ("gain_and_band_pass", (222, 428))])
def test_reference_goldens_through_a_live_batch(ra, ctx, case, chunks, pieces):
    """tests/detector.rs:112-162 with the filters inside a live-stream batch: the detections the reference asserts, in the chunks the
    oracle's chunk-wise detector reports them, and every field of them bit for bit what rp_frontend_batch -> rp_batch_detect finds
    over the whole stream."""
    e = EXP["simulation"][case]
    w = rpw_py.load_rpw(os.path.join(G, e["rpw"]))
    templates = list(w["samples_features"].values())
    s16 = simstream.simulation_stream_i16(*e.get("gains", [1.0, 1.0]))
    n = (len(s16) // 480) * 480
    cfg = _golden_config(ra, e)
    tm = ra.Templates(ctx, templates, avg=w["avg_features"])
    out, _, _ = ctx.frontend(s16[:n], cfg.filters, w["rms_level"], tm.max_len // 3)
    det, n_det = ctx.batch_detect(out, tm, cfg.detector)
    sb = ra.StreamBatch(ctx, tm, cfg.detector, 1, max_chunks_per_call=max(pieces), filters=cfg.filters, rms_level_ref=w["rms_level"])
    got, _, _, _ = _feed(sb, s16[None, :n], pieces, want_agg=False)
    assert len(got[0]) == n_det[0] == len(e["detections"]) == 2
    for j, (_, gscore) in enumerate(e["detections"]):
        print(case, pieces, j, _det_tuple(got[0][j]), gscore)
        assert _same(got[0][j], det[0][j])
        assert got[0][j]["frame"] // 3 + 1 == chunks[j]
        assert abs(got[0][j]["score"] - np.float32(gscore)) <= 1e-5 * gscore


def _varying_noise(S, n_chunks, rng):
    """Gaussian noise whose amplitude changes every 6 chunks, log-uniform in 0.01 .. 0.6, clipped to +-1; stream 3 silent"""
    pcm = np.empty((S, n_chunks * 480), np.float32)
    for s in range(S):
        for c0 in range(0, n_chunks, 6):
            amp = np.exp(rng.uniform(np.log(0.01), np.log(0.6)))
            m = min(6, n_chunks - c0) * 480
            pcm[s, c0 * 480:c0 * 480 + m] = np.clip(rng.standard_normal(m) * amp, -1.0, 1.0).astype(np.float32)
    pcm[3] = 0
    return pcm


def _as_format(pcm, dtype):
    """-> (the array fed to the device, the f32 samples the reference's decode makes of it)"""
    if dtype == np.float32:
        return pcm, pcm
    if dtype == np.int16:
        raw = np.round(pcm * 32767.0).astype(np.int16)
        return raw, raw.astype(np.float32) / np.float32(32767.0)
    if dtype == np.int8:
        raw = np.round(pcm * 127.0).astype(np.int8)
        return raw, raw.astype(np.float32) / np.float32(127.0)
    raw = np.round(pcm.astype(np.float64) * 2147483647.0).astype(np.int32)
    return raw, raw.astype(np.float32) / np.float32(2147483648.0)   # v as f32 / i32::MAX as f32 (= 2^31)


@pytest.mark.parametrize("dtype,pieces", [(np.int16, (1,)), (np.int16, (3, 1, 2)), (np.int16, (4,)), (np.float32, (1,)), (np.float32, (3, 1, 2)),
                                          (np.float32, (4,)), (np.int8, (3, 1, 2)), (np.int32, (4,))])
def test_state_carried_across_calls(ra, ctx, dtype, pieces):
    """70 streams (a partial last workgroup) x 60 chunks of noise whose loudness keeps changing, gain normaliser (window of 7 levels)
    and band-pass both working: every call's levels() equal to the oracle's front-end over the whole stream, and every window's
    aggregate equal to rp_frontend_batch -> rp_batch_detect over the whole stream, bit for bit, for all streams."""
    S, NC = 70, 60
    pcm, dec = _as_format(_varying_noise(S, NC, np.random.default_rng(8)), dtype)
    f = _filters(ra, True, True, 0.2, 3.0, 120.0, 900.0)
    templates = orc.synth_templates(SEED, 4, 22, 5)
    tm = ra.Templates(ctx, templates)
    assert tm.max_len // 3 == 7
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold, cfg.min_scores = 0.0, 0.3, 2
    out, _, _ = ctx.frontend(pcm, f, 0.05, 7)
    det, n_det, _, agg = ctx.batch_detect(out, tm, cfg, want_scores=True)
    sb = ra.StreamBatch(ctx, tm, cfg, S, max_chunks_per_call=max(pieces), filters=f, rms_level_ref=0.05)
    got, live_agg, rms, gains = _feed(sb, pcm, pieces)
    checked = (0, 3, 69, 1, 17, 33, 63, 64, 68)
    all_gains = []
    for s in checked:
        _, rr, rg = orc.frontend_stream(dec[s], gain_normalizer=True, min_gain=0.2, max_gain=3.0, rms_level_ref=0.05, window_size=7,
                                        band_pass=True, low_cutoff=120.0, high_cutoff=900.0)
        assert np.array_equal(rms[s].view(np.uint32), rr.view(np.uint32)), s
        assert np.array_equal(gains[s].view(np.uint32), rg.view(np.uint32)), s
        if s != 3:
            all_gains.append(rg)
    assert np.all(gains[3] == 1.0) and np.all(rms[3] == 0.0)
    all_gains = np.concatenate(all_gains)
    share, distinct = float(np.mean(all_gains != 1.0)), len(np.unique(all_gains))
    print("gains != 1 in %.2f of the chunks, %d distinct values" % (share, distinct))
    assert share >= 0.5 and distinct >= 8   # the filters do real work
    assert _agg_equal_offline(live_agg, agg, tm.max_len) >= 3 * NC - tm.max_len - 3
    for s in range(S):
        assert len(got[s]) == n_det[s]
        assert [_det_tuple(d) for d in got[s]][:8] == [_det_tuple(det[s][j]) for j in range(min(n_det[s], 8))]


def test_against_the_chunkwise_oracle_detector_with_resets(ra, ctx):
    """Streams of the golden utterances at different loudness through a live batch and, one by one, through the oracle's Rustpotter
    mirror with both filters on; one stream is reset in the middle of an utterance on both sides.  Same detections (chunk and counter
    exact, scores to 1e-5), the gain a detection reports = the gain of the chunk in which its best window was scored, and the reset
    stream's levels go on as if nothing had happened (Rustpotter::reset leaves the filters alone)."""
    w = rpw_py.load_rpw(os.path.join(G, "oye_casa_g.rpw"))
    templates = list(w["samples_features"].values())
    rng = np.random.default_rng(31)
    streams = []
    for g1, g2 in ((0.2, 5.0), (0.5, 2.0), (1.0, 0.3), (0.5, 2.0)):
        s = simstream.simulation_stream_i16(g1, g2)
        streams.append((s.astype(np.int32) + rng.integers(-12, 13, len(s))).clip(-32768, 32767).astype(np.int16))
    streams[3] = streams[1].copy()   # stream 3 = stream 1 without the reset
    n = (len(streams[0]) // 480) * 480
    pcm = np.stack([s[:n] for s in streams])
    kw = dict(gain_normalizer=True, min_gain=0.2, max_gain=4.0, band_pass=True, low_cutoff=80.0, high_cutoff=500.0)
    f = _filters(ra, True, True, 0.2, 4.0, 80.0, 500.0)
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold = 0.0, 0.5
    tm = ra.Templates(ctx, templates, avg=w["avg_features"])
    reset_chunk = 185   # the first utterance spans chunks 167 .. 200
    sb = ra.StreamBatch(ctx, tm, cfg, len(streams), max_chunks_per_call=3, filters=f, rms_level_ref=w["rms_level"])
    got, _, rms, gains = _feed(sb, pcm, (1,), want_agg=False, before_call=lambda c: sb.reset(1) if c == reset_chunk else None)
    total = 0
    for s in range(len(streams)):
        d = orc.Detector(avg_threshold=0.0, threshold=0.5, **kw)
        d.add_ref(w)
        want = []
        for c in range(n // 480):
            if s == 1 and c == reset_chunk:
                d.reset()
            r = d.process_i16(pcm[s, c * 480:(c + 1) * 480])
            if r is not None:
                want.append((c, r))
        assert len(got[s]) == len(want), (s, len(got[s]), len(want))
        for rec, (chunk, r) in zip(got[s], want):
            best_chunk = (int(rec["window"]) + tm.max_len - 1) // 3 + 1
            print(s, chunk, r["counter"], float(r["score"]), float(rec["score"]), float(r["gain"]), float(gains[s][best_chunk]))
            assert rec["frame"] // 3 + 1 == chunk and rec["counter"] == r["counter"]
            assert abs(rec["score"] - r["score"]) <= 1e-5 * r["score"]
            assert gains[s][best_chunk] == r["gain"]
        total += len(want)
        _, rr, rg = orc.frontend_stream(simstream.i16_to_f32(pcm[s]), rms_level_ref=w["rms_level"], window_size=tm.max_len // 3, **kw)
        assert np.array_equal(rms[s], rr) and np.array_equal(gains[s], rg), s
    assert total >= 4
    assert len(got[1]) < len(got[3])                                              # the reset cost stream 1 a detection ...
    assert np.array_equal(rms[1], rms[3]) and np.array_equal(gains[1], gains[3])  # ... and left its filters alone
    assert len(np.unique(np.concatenate([gains[s] for s in range(3)]))) >= 8


def test_48k_input_with_filters(ra, ctx):
    """tests/detector.rs:188-213 (real_sample.wav at 48 kHz, min_gain 0.4, band 210-700 Hz) through a live batch of 48 kHz streams, two
    chunks per call: the per-call resampler + filters + streaming path == rp_resample_batch -> rp_frontend_batch -> rp_batch_detect
    over the whole stream, every aggregate and every detection bit for bit."""
    e = EXP["audio_file"]["noise_filters"]
    w = rpw_py.load_rpw(os.path.join(G, e["rpw"]))
    pcm48, sr, _ = rpw_py.read_wav(os.path.join(G, e["wav"]))
    assert sr == 48000
    n = (len(pcm48) // 2880) * 2880
    x = np.asarray(pcm48[:n], np.float32)
    streams = np.stack([x, np.roll(x, 1440 * 9), x * np.float32(0.5)])
    cfg = _golden_config(ra, e)
    tm = ra.Templates(ctx, list(w["samples_features"].values()), avg=w["avg_features"])
    mono16 = ctx.resample(streams, 48000)
    out, _, _ = ctx.frontend(mono16, cfg.filters, w["rms_level"], tm.max_len // 3)
    det, n_det, _, agg = ctx.batch_detect(out, tm, cfg.detector, want_scores=True)
    assert n_det[0] >= 2
    sb = ra.StreamBatch(ctx, tm, cfg.detector, 3, max_chunks_per_call=2, sample_rate=48000, filters=cfg.filters, rms_level_ref=w["rms_level"])
    assert sb.samples_per_chunk == 1440
    got, live_agg, rms, gains = _feed(sb, streams, (2,), spc=1440)
    assert _agg_equal_offline(live_agg, agg, tm.max_len) >= agg.shape[1] - 3
    for s in range(3):
        assert [_det_tuple(d) for d in got[s]] == [_det_tuple(det[s][j]) for j in range(n_det[s])]
    assert np.any(gains != 1.0)


def _two_wakeword_streams():
    rd = lambda f: simstream.i16_to_f32(rpw_py.read_wav_i16(os.path.join(G, f))[0])
    z = np.zeros(16000 * 2, np.float32)
    base = np.concatenate([z, rd("oye_casa_g_1.wav"), z, rd("alexa.wav"), z, rd("oye_casa_g_2.wav"), z, rd("alexa2.wav"), z, z])
    rng = np.random.default_rng(12)
    n = (len(base) // 480) * 480
    return np.stack([base[:n], np.roll(base[:n], 480 * 13) + rng.standard_normal(n).astype(np.float32) * np.float32(0.001),
                     np.roll(base[:n], 480 * 41)])


def _feed_multi(sb, pcm, pieces, max_det=4):
    S, N = pcm.shape
    out = [[] for _ in range(S)]
    pos, k = 0, 0
    while pos < N:
        nc = min(pieces[k % len(pieces)], (N - pos) // 480)
        k += 1
        det, dww, dlab, n_det = sb.process_multi(pcm[:, pos:pos + 480 * nc], max_det=max_det)
        pos += 480 * nc
        for s in range(S):
            for j in range(n_det[s]):
                out[s].append((det[s][j].copy(), int(dww[s][j]), int(dlab[s][j])))
    return out


@pytest.mark.parametrize("pieces", PIECES)
def test_several_wakewords_with_filters(ra, ctx, pieces):
    """rp_stream_batch_new_multi with two wakeword references and both filters: the detections and firing wakewords of
    rp_frontend_batch -> rp_batch_detect_multi over the whole stream, bit for bit; the gain window follows the longest wakeword."""
    pcm = _two_wakeword_streams() * np.float32(0.4)
    wws = [rpw_py.load_rpw(os.path.join(G, f)) for f in ("oye_casa_g.rpw", "alexa.rpw")]
    tms = [ra.Templates(ctx, list(w["samples_features"].values()), avg=w["avg_features"]) for w in wws]
    ref = max(w["rms_level"] for w in wws)
    window = max(t.max_len for t in tms) // 3
    f = _filters(ra, True, True, 0.5, 3.0, 80.0, 1200.0)
    cfg = ra.DetectorConfig()
    cfg.threshold, cfg.avg_threshold, cfg.min_scores = 0.5, 0.2, 3
    out, _, want_gains = ctx.frontend(pcm, f, ref, window)
    det, dww, n_det = ctx.batch_detect_multi(out, tms, cfg)
    sb = ra.StreamBatch(ctx, None, cfg, pcm.shape[0], max_chunks_per_call=max(pieces), mfcc_size=5,
                        wakewords=[{"templates": tms[0]}, {"templates": tms[1]}], filters=f, rms_level_ref=ref)
    got = _feed_multi(sb, pcm, pieces)
    print("detections per stream", n_det, "share of gains != 1", float(np.mean(want_gains != 1.0)))
    for s in range(pcm.shape[0]):
        assert len(got[s]) == n_det[s], (s, len(got[s]), n_det[s])
        for j, (rec, ww, lab) in enumerate(got[s]):
            assert _same(rec, det[s][j]) and ww == dww[s][j] and lab == -1
    assert n_det.sum() >= 2 and np.mean(want_gains != 1.0) > 0.05


def test_off_means_off(ra, ctx):
    """A batch that never had rp_stream_batch_set_filters, one that had it with both filters disabled, and the whole-stream call:
    identical detections and aggregates, bit for bit (16 kHz mono read in place, and stereo input through the staged rows); the
    batch with disabled filters still reports every chunk's RMS level, and gains of exactly 1."""
    pcm = _two_wakeword_streams()
    wws = [rpw_py.load_rpw(os.path.join(G, f)) for f in ("oye_casa_g.rpw", "alexa.rpw")]
    tms = [ra.Templates(ctx, list(w["samples_features"].values()), avg=w["avg_features"]) for w in wws]
    cfg = ra.DetectorConfig()
    cfg.threshold, cfg.avg_threshold, cfg.min_scores = 0.5, 0.2, 3
    off = _filters(ra)
    S = pcm.shape[0]
    ref_levels = [orc.frontend_stream(pcm[s])[1] for s in range(S)]
    # one reference
    det, n_det, _, agg = ctx.batch_detect(pcm, tms[0], cfg, want_scores=True)
    assert n_det.sum() >= 3
    plain = ra.StreamBatch(ctx, tms[0], cfg, S, max_chunks_per_call=3)
    unset = ra.StreamBatch(ctx, tms[0], cfg, S, max_chunks_per_call=3, filters=off, rms_level_ref=0.05)
    with pytest.raises(ra.RustpotterError):
        plain.levels()   # no filters configured: nothing is kept
    g0, a0, _, _ = _feed(plain, pcm, (3, 1, 2), levels=False)
    g1, a1, rms, gains = _feed(unset, pcm, (3, 1, 2))
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
    assert _agg_equal_offline(a1, agg, tms[0].max_len) >= agg.shape[1] - 3
    for s in range(S):
        assert [_det_tuple(d) for d in g0[s]] == [_det_tuple(d) for d in g1[s]] == [_det_tuple(det[s][j]) for j in range(n_det[s])]
        assert np.array_equal(rms[s].view(np.uint32), ref_levels[s].view(np.uint32))
    assert np.all(gains == 1.0)
    # the same streams as the left channel of stereo input: the staged rows
    inter = np.stack([pcm, np.full_like(pcm, 0.25)], axis=2).reshape(S, -1)
    plain = ra.StreamBatch(ctx, tms[0], cfg, S, max_chunks_per_call=3, channels=2)
    unset = ra.StreamBatch(ctx, tms[0], cfg, S, max_chunks_per_call=3, channels=2, filters=off)
    g2, a2, _, _ = _feed(plain, inter, (3, 1, 2), levels=False, spc=960)
    g3, a3, rms, gains = _feed(unset, inter, (3, 1, 2), spc=960)
    assert np.array_equal(a2.view(np.uint32), a3.view(np.uint32)) and np.array_equal(a2.view(np.uint32), a0.view(np.uint32))
    for s in range(S):
        assert [_det_tuple(d) for d in g2[s]] == [_det_tuple(d) for d in g3[s]] == [_det_tuple(d) for d in g0[s]]
        assert np.array_equal(rms[s].view(np.uint32), ref_levels[s].view(np.uint32))
    assert np.all(gains == 1.0)
    # two wakewords
    det, dww, n_det = ctx.batch_detect_multi(pcm, tms, cfg)
    specs = [{"templates": tms[0]}, {"templates": tms[1]}]
    plain = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=3, mfcc_size=5, wakewords=specs)
    unset = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=3, mfcc_size=5, wakewords=specs, filters=off)
    m0, m1 = _feed_multi(plain, pcm, (3, 1, 2)), _feed_multi(unset, pcm, (3, 1, 2))
    for s in range(S):
        assert len(m0[s]) == len(m1[s]) == n_det[s]
        for j in range(n_det[s]):
            assert _same(m0[s][j][0], det[s][j]) and _same(m1[s][j][0], det[s][j]) and m0[s][j][1] == m1[s][j][1] == dww[s][j]
    lr, lg = unset.levels()
    assert np.all(lg == 1.0) and np.array_equal(lr[:, -1], np.array([r[-1] for r in ref_levels]))


def test_refusals_leave_the_batch_as_it_was(ra, ctx):
    """set_filters after audio, filters together with 40 ms input frames (either order), levels() before any audio: each is refused
    with a message, and the batch goes on exactly like a twin that never saw the refused call."""
    tm = ra.Templates(ctx, orc.synth_templates(SEED, 4, 22, 5))
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold, cfg.min_scores = 0.0, 0.3, 2
    f = _filters(ra, True, True, 0.2, 3.0, 120.0, 900.0)
    S = 5
    pcm = _varying_noise(S, 12, np.random.default_rng(3))

    def same_run(a, b, x, spc=480, levels=True):
        ra_, rb = _feed(a, x, (2, 1), spc=spc, levels=levels), _feed(b, x, (2, 1), spc=spc, levels=levels)
        assert np.array_equal(ra_[1].view(np.uint32), rb[1].view(np.uint32))
        for s in range(S):
            assert [_det_tuple(d) for d in ra_[0][s]] == [_det_tuple(d) for d in rb[0][s]]
        if levels:
            assert np.array_equal(ra_[2], rb[2]) and np.array_equal(ra_[3], rb[3])

    # after the first process call
    a, twin = ra.StreamBatch(ctx, tm, cfg, S, max_chunks_per_call=2), ra.StreamBatch(ctx, tm, cfg, S, max_chunks_per_call=2)
    a.process(pcm[:, :480]); twin.process(pcm[:, :480])
    with pytest.raises(ra.RustpotterError, match="already received audio"):
        a.set_filters(f, 0.05)
    with pytest.raises(ra.RustpotterError):
        a.levels()
    same_run(a, twin, pcm[:, 480:], levels=False)
    # filters, then 22.05 kHz input
    a = ra.StreamBatch(ctx, tm, cfg, S, max_chunks_per_call=2, filters=f, rms_level_ref=0.05)
    twin = ra.StreamBatch(ctx, tm, cfg, S, max_chunks_per_call=2, filters=f, rms_level_ref=0.05)
    with pytest.raises(ra.RustpotterError, match="40 ms"):
        a.set_input(22050)
    with pytest.raises(ra.RustpotterError, match="not received audio"):
        a.levels()
    assert a.samples_per_chunk == 480
    same_run(a, twin, pcm)
    # 22.05 kHz input, then filters
    a = ra.StreamBatch(ctx, tm, cfg, S, max_chunks_per_call=2, sample_rate=22050)
    twin = ra.StreamBatch(ctx, tm, cfg, S, max_chunks_per_call=2, sample_rate=22050)
    with pytest.raises(ra.RustpotterError, match="40 ms"):
        a.set_filters(f, 0.05)
    assert a.samples_per_chunk == 882 and a.frames_per_chunk == 4
    x = _varying_noise(S, 24, np.random.default_rng(4))[:, :882 * 12]
    same_run(a, twin, x, spc=882, levels=False)
    # set_input to another 30 ms rate after filters is fine, in either order
    b1 = ra.StreamBatch(ctx, tm, cfg, S, max_chunks_per_call=2, filters=f, rms_level_ref=0.05)
    b1.set_input(48000)
    b2 = ra.StreamBatch(ctx, tm, cfg, S, max_chunks_per_call=2, sample_rate=48000, filters=f, rms_level_ref=0.05)
    x = _varying_noise(S, 36, np.random.default_rng(5))[:, :1440 * 12]
    same_run(b1, b2, x, spc=1440)
