"""The gain normaliser on personal-wakeword batches: every stream works towards the rms_level of ITS wakeword of a bank over that wakeword's
window of max_len / 3 chunk levels -- rp_frontend_batch_bank over whole streams (gain_per_stream_kernel) and rp_stream_batch_set_filters_bank
on live streams (stream_filters_kernel, per-stream form), with rp_wakeword_bank_set_rms_levels / rp_wakeword_bank_rms_level.  Checked bit for
bit against the CPU oracle's front-end per stream, live against whole, against the oracle's chunk-wise detector with slots that change
wakeword, and against the shared-wakeword calls when every stream indexes the same wakeword."""
import ctypes as C
import os

import numpy as np
import pytest

import rpw_py
import simstream
from oracle import rp_oracle as orc

pytestmark = pytest.mark.gpu

G = simstream.GOLDEN
SEED = 0x5EED00000BF17E55
GOLDEN_RPW = ["alexa.rpw", "oye_casa_g.rpw", "oye_casa_real.rpw"]   # window lengths 126 / 108 / 168: gain windows 42 / 36 / 56
# the synthetic wakewords behind the goldens: (template length, rms_level) -> gain windows 7, 7, 1, 2, 0 -> 1, 7
SYNTH = [(22, 0.05), (22, 0.01), (4, 0.05), (7, 0.05), (2, 0.05), (22, float("nan"))]
WINDOWS = [42, 36, 56, 7, 7, 1, 2, 1, 7]
NAN_W = 8
S, NC = 70, 90
MIN_GAIN, MAX_GAIN = 0.2, 3.0
LOW, HIGH = 120.0, 900.0
PIECES = [(1,), (3, 1, 2), (4,)]


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


def filters(ra, gain=True, band=True, gain_ref=None, min_gain=MIN_GAIN, max_gain=MAX_GAIN, low=LOW, high=HIGH):
    f = ra.FiltersConfig()
    f.gain_normalizer.enabled, f.gain_normalizer.min_gain, f.gain_normalizer.max_gain = gain, min_gain, max_gain
    f.gain_normalizer.gain_ref = gain_ref
    f.band_pass.enabled, f.band_pass.low_cutoff, f.band_pass.high_cutoff = band, low, high
    return f


def synth_dicts():
    out = []
    for j, (L, level) in enumerate(SYNTH):
        tm = orc.synth_templates(SEED + 100 * j, 3, L, 5)
        out.append({"name": "synth%d" % j, "samples_features": {"t%d" % t: m for t, m in enumerate(tm)}, "avg_features": None, "threshold": None,
                    "avg_threshold": None, "rms_level": level, "mfcc_size": 5})
    return out


def bank_rpw():
    return [read(n) for n in GOLDEN_RPW] + [rpw_py.dump_rpw_ref(d["name"], d["samples_features"], rms_level=d["rms_level"]) for d in synth_dicts()]


def make_bank(ra, ctx):
    bank = ra.WakewordBank(ctx, rpw=bank_rpw())
    assert [max(L // 3, 1) for L in bank.max_lens] == WINDOWS and bank.W == 9
    return bank


@pytest.fixture(scope="module")
def dicts():
    return [rpw_py.load_rpw(os.path.join(G, n)) for n in GOLDEN_RPW] + synth_dicts()


@pytest.fixture(scope="module")
def bank(ra, ctx, dicts):
    b = make_bank(ra, ctx)
    lv = b.rms_levels
    want = np.array([d["rms_level"] for d in dicts], np.float32)
    assert np.array_equal(bits(lv[:NAN_W]), bits(want[:NAN_W])) and np.isnan(lv[NAN_W])   # what the files hold: 0.0575 / 0.0526 / 0.0099 / ...
    return b


def varying_noise(n_streams, n_chunks, rng, silent=3):
    """Gaussian noise whose amplitude changes every 6 chunks, log-uniform in 0.01 .. 0.6, clipped to +-1; stream `silent` silent"""
    pcm = np.empty((n_streams, n_chunks * 480), np.float32)
    for s in range(n_streams):
        for c0 in range(0, n_chunks, 6):
            amp = np.exp(rng.uniform(np.log(0.01), np.log(0.6)))
            m = min(6, n_chunks - c0) * 480
            pcm[s, c0 * 480:c0 * 480 + m] = np.clip(rng.standard_normal(m) * amp, -1.0, 1.0).astype(np.float32)
    if silent is not None:
        pcm[silent] = 0
    return pcm


def as_format(pcm, dtype):
    """-> (the array fed to the device, the f32 samples the reference's decode makes of it)"""
    if dtype == np.float32:
        return pcm, pcm
    raw = np.round(pcm * 32767.0).astype(np.int16)
    return raw, raw.astype(np.float32) / np.float32(32767.0)


@pytest.fixture(scope="module")
def audio():
    """streams 0..9 all carry stream 0's audio, with wakewords 0..8 and -1; the others their own audio and wakeword s % 10 - 1; stream 20
    (no wakeword: nothing scores its all-equal frames) is silent -- a silent stream WITH a wakeword is in test_stream_counts_and_a_short_tail"""
    pcm = varying_noise(S, NC, np.random.default_rng(8), silent=20)
    pcm[1:10] = pcm[0]
    idx = np.array([s if s < 9 else -1 for s in range(10)] + [s % 10 - 1 for s in range(10, S)], np.int32)
    return pcm, idx


def oracle_rows(dec, idx, dicts, band, gain_ref=None):
    """orc.frontend_stream per stream with its wakeword's level and window -> (out, rms, gains) as [S][..] arrays"""
    out, rms, gains = [], [], []
    memo = {}
    for s in range(dec.shape[0]):
        w = int(idx[s])
        key = (dec[s].tobytes(), w)
        if key not in memo:
            if w < 0:   # a detector without wakewords: gain 1; the band-pass runs as on a live bank batch
                memo[key] = orc.frontend_stream(dec[s], band_pass=band, low_cutoff=LOW, high_cutoff=HIGH)
            else:
                L = max(len(t) for t in dicts[w]["samples_features"].values())
                memo[key] = orc.frontend_stream(dec[s], gain_normalizer=True, gain_ref=gain_ref, min_gain=MIN_GAIN, max_gain=MAX_GAIN,
                                                rms_level_ref=dicts[w]["rms_level"], window_size=L // 3, band_pass=band, low_cutoff=LOW, high_cutoff=HIGH)
        o, r, g = memo[key]
        out.append(o); rms.append(r); gains.append(g)
    return np.stack(out), np.stack(rms), np.stack(gains)


_ORACLE = {}


def oracle_case(audio, dicts, dtype, band, gain_ref=None):
    key = (np.dtype(dtype).name, band, gain_ref)
    if key not in _ORACLE:
        pcm, idx = audio
        raw, dec = as_format(pcm, dtype)
        _ORACLE[key] = (raw,) + oracle_rows(dec, idx, dicts, band, gain_ref)
    return _ORACLE[key]


# ---------------------------------------------------------------------------------------------- 1. whole streams against the oracle

@pytest.mark.parametrize("dtype,band", [(np.float32, True), (np.float32, False), (np.int16, True), (np.int16, False)])
def test_whole_streams_against_the_oracle(ra, ctx, bank, dicts, audio, dtype, band):
    """1. 70 streams (a partial last wave) x 90 chunks: rms, gains and the filtered samples of rp_frontend_batch_bank equal, as uint32,
    orc.frontend_stream with the stream's own rms_level_ref and window_size, for every stream."""
    _, idx = audio
    raw, want_out, want_rms, want_gains = oracle_case(audio, dicts, dtype, band)
    out, rms, gains = ctx.frontend_bank(raw, filters(ra, True, band), bank, idx)
    # the conditions that keep the test honest, on the oracle's rows: the seven stream-0 copies with a (level, window) of their own
    rows = want_gains[:7]
    for a in range(7):
        share = float(np.mean(rows[a] != 1.0))
        assert share >= 0.5, (a, share)
        for b in range(a + 1, 7):
            assert int(np.sum(rows[a] != rows[b])) >= 10, (a, b, int(np.sum(rows[a] != rows[b])))
    assert np.all(want_gains[idx < 0] == 1.0) and np.all(want_gains[idx == NAN_W] == 1.0) and np.all(want_rms[20] == 0.0)
    for s in range(S):
        assert np.array_equal(bits(rms[s]), bits(want_rms[s])), s
        assert np.array_equal(bits(gains[s]), bits(want_gains[s])), (s, int(idx[s]), int(np.sum(gains[s] != want_gains[s])))
        assert np.array_equal(bits(out[s]), bits(want_out[s])), (s, int(idx[s]))


def test_whole_streams_with_a_fixed_gain_ref(ra, ctx, bank, dicts, audio):
    """1. has_gain_ref: one reference level for all streams, the window still per stream -- the alexa and oye_casa_g copies of stream 0
    (windows 42 / 36) differ."""
    _, idx = audio
    raw, want_out, want_rms, want_gains = oracle_case(audio, dicts, np.float32, True, 0.05)
    assert int(np.sum(want_gains[0] != want_gains[1])) >= 10
    assert np.all(want_gains[idx < 0] == 1.0) and np.any(want_gains[idx == NAN_W] != 1.0)   # a fixed level serves a wakeword without one
    out, rms, gains = ctx.frontend_bank(raw, filters(ra, True, True, gain_ref=0.05), bank, idx)
    assert np.array_equal(bits(rms), bits(want_rms)) and np.array_equal(bits(gains), bits(want_gains)) and np.array_equal(bits(out), bits(want_out))


# ---------------------------------------------------------------------------------------------- 2. live = whole

def feed(sb, pcm, pieces, want_agg=False, before_chunk=None, max_det=8):
    """pcm [S][C * 480] through the batch in calls of pieces[i % len] chunks -> (detections per stream as (frame, window, counter, score bits,
    avg bits), agg [S][frames] or None, rms [S][C], gains [S][C]); before_chunk(c) runs ahead of the call that starts with chunk c"""
    n_streams, total = pcm.shape[0], pcm.shape[1] // 480
    got, aggs, rms, gains = [[] for _ in range(n_streams)], [], [], []
    c = k = 0
    while c < total:
        n = min(pieces[k % len(pieces)], total - c)
        k += 1
        if before_chunk is not None:
            before_chunk(c)
        r = sb.process(np.ascontiguousarray(pcm[:, c * 480:(c + n) * 480]), max_det=max_det, want_agg=want_agg)
        for s in range(n_streams):
            assert r[1][s] <= max_det
            for d in r[0][s][:r[1][s]]:
                got[s].append((int(d["frame"]), int(d["window"]), int(d["counter"]), bits1(d["score"]), bits1(d["avg_score"])))
        if want_agg:
            aggs.append(r[2].copy())
        lr, lg = sb.levels()
        assert lr.shape == (n_streams, n) and lg.shape == (n_streams, n)
        rms.append(lr); gains.append(lg)
        c += n
    return got, (np.concatenate(aggs, axis=1) if want_agg else None), np.concatenate(rms, axis=1), np.concatenate(gains, axis=1)


def live_config(ra):
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold, cfg.min_scores = 0.0, 0.3, 2
    return cfg


def same_aggregates(bank, idx, live_agg, whole_agg, fpc=3):
    """the live aggregate at frame f >= max_len(s) - 1 is the whole call's agg[s][f - max_len(s) + 1]; column j of the live rows is frame j - fpc"""
    n = 0
    for s, w in enumerate(idx):
        if w < 0:
            assert not live_agg[s].any(), s
            continue
        L = bank.max_lens[w]
        f = np.arange(L - 1, live_agg.shape[1] - fpc)
        a, b = bits(live_agg[s][f + fpc]), bits(whole_agg[s][f - L + 1])
        assert np.array_equal(a, b), (s, w, "agg differs in %d of %d windows" % (int(np.sum(a != b)), len(f)))
        n += len(f)
    return n


_WHOLE = {}


def whole_detect(ra, ctx, bank, audio, dtype):
    """rp_frontend_batch_bank -> rp_batch_detect_bank over the whole streams, once per input format"""
    key = np.dtype(dtype).name
    if key not in _WHOLE:
        pcm, idx = audio
        raw, _ = as_format(pcm, dtype)
        out, _, _ = ctx.frontend_bank(raw, filters(ra), bank, idx)
        det, n_det, agg, _ = ctx.batch_detect_bank(out, bank, idx, live_config(ra), max_det=32, want_agg=True)
        _WHOLE[key] = ([[(int(d["frame"]), int(d["window"]), int(d["counter"]), bits1(d["score"]), bits1(d["avg_score"])) for d in det[s][:n_det[s]]]
                        for s in range(S)], agg)
    return _WHOLE[key]


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("pieces", PIECES)
def test_live_equals_whole(ra, ctx, bank, dicts, audio, pieces, dtype):
    """2. The same bank and streams fed in pieces: every call's levels() are test 1's rows bit for bit, every aggregate of a window that
    lies inside the stream and every detection those of rp_frontend_batch_bank -> rp_batch_detect_bank over the whole stream."""
    pcm, idx = audio
    raw, _, want_rms, want_gains = oracle_case(audio, dicts, dtype, True)
    before = ctx.dtw_ref_pairs()
    want_det, want_agg = whole_detect(ra, ctx, bank, audio, dtype)
    sb = ra.StreamBatch(ctx, None, live_config(ra), S, max_chunks_per_call=max(pieces), bank=bank, stream_wakeword=idx, bank_filters=filters(ra))
    got, agg, rms, gains = feed(sb, raw, pieces, want_agg=True)
    assert ctx.dtw_ref_pairs() == before
    assert np.array_equal(bits(rms), bits(want_rms))
    assert np.array_equal(bits(gains), bits(want_gains)), np.argwhere(gains != want_gains)[:8]
    assert same_aggregates(bank, idx, agg, want_agg) > 0
    for s in range(S):
        assert got[s] == want_det[s], (s, got[s], want_det[s])


# ---------------------------------------------------------------------------------------------- 3. the oracle's detector, slot changes

def utterances(files, g1, g2, rng):
    """simstream.simulation_stream_i16 for any two recordings: 5 s of silence around each, the recordings at gains g1 / g2, +-12 of dither"""
    z = np.zeros(16000 * 5, np.int16)
    a, b = (simstream._read_raw(os.path.join(G, f), g) for f, g in zip(files, (g1, g2)))
    s = np.concatenate([z, a, z, b, z])
    return (s.astype(np.int32) + rng.integers(-12, 13, len(s))).clip(-32768, 32767).astype(np.int16)


DET_KW = dict(gain_normalizer=True, min_gain=0.2, max_gain=4.0, band_pass=True, low_cutoff=80.0, high_cutoff=500.0)


def test_against_the_chunkwise_oracle_detector(ra, ctx, bank, dicts):
    """3. Streams of the golden utterances at different loudness, carrying oye_casa_g or alexa, both filters on, through a live batch over
    the bank and one by one through orc.Detector with that wakeword: same detections (chunk and counter exact, scores to 1e-5), the gain
    of the best window's chunk is the oracle's gain, the levels equal the oracle's front-end with the wakeword's own level and window."""
    rng = np.random.default_rng(31)
    oye, alexa = ("oye_casa_g_1.wav", "oye_casa_g_2.wav"), ("alexa.wav", "alexa2.wav")
    plan = [(oye, 1, 0.2, 5.0), (oye, 1, 0.5, 2.0), (alexa, 0, 0.5, 2.0), (alexa, 0, 1.0, 0.3), (oye, 0, 0.5, 2.0)]
    streams = [utterances(f, g1, g2, rng) for f, _, g1, g2 in plan]
    n = (min(len(s) for s in streams) // 480) * 480
    pcm = np.stack([s[:n] for s in streams])
    idx = [w for _, w, _, _ in plan]
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold = 0.0, 0.5
    f = filters(ra, True, True, min_gain=0.2, max_gain=4.0, low=80.0, high=500.0)
    sb = ra.StreamBatch(ctx, None, cfg, len(plan), max_chunks_per_call=3, bank=bank, stream_wakeword=idx, bank_filters=f)
    got, _, rms, gains = feed(sb, pcm, (3,))
    fired = set()
    total = 0
    for s, w in enumerate(idx):
        d = orc.Detector(avg_threshold=0.0, threshold=0.5, **DET_KW)
        d.add_ref(dicts[w])
        want = [(c, r) for c in range(n // 480) for r in [d.process_i16(pcm[s, c * 480:(c + 1) * 480])] if r is not None]
        assert len(got[s]) == len(want), (s, got[s], want)
        for rec, (chunk, r) in zip(got[s], want):
            score = np.array([rec[3]], np.uint32).view(np.float32)[0]
            best_chunk = (rec[1] + bank.max_lens[w] - 1) // 3 + 1
            print(s, w, chunk, r["counter"], float(r["score"]), float(score), float(r["gain"]), float(gains[s][best_chunk]))
            assert rec[0] // 3 + 1 == chunk and rec[2] == r["counter"]
            assert abs(score - r["score"]) <= 1e-5 * r["score"]
            assert gains[s][best_chunk] == r["gain"]
            fired.add(w)
        total += len(want)
        _, rr, rg = orc.frontend_stream(simstream.i16_to_f32(pcm[s]), rms_level_ref=dicts[w]["rms_level"], window_size=bank.max_lens[w] // 3, **DET_KW)
        assert np.array_equal(bits(rms[s]), bits(rr)) and np.array_equal(bits(gains[s]), bits(rg)), s
    assert total >= 4 and fired == {0, 1}, (total, fired)


def detector_gains(d, dec, actions=None, skip=()):
    """feeds orc.Detector the stream chunk by chunk (actions[c](d) ahead of chunk c; chunks in `skip` are not fed) -> [(chunk, detection)]"""
    out = []
    for c in range(len(dec) // 480):
        if actions and c in actions:
            actions[c](d)
        if c in skip:
            continue
        r = d.process_f32(dec[c * 480:(c + 1) * 480])
        if r is not None:
            out.append((c, r))
    return out


def test_slots_keep_their_window(ra, ctx, bank, dicts):
    """3. On noise, gain normaliser alone.  (a) stream 0 goes from oye_casa_real (window 56) to a 22-frame wakeword (window 7) at chunk 60:
    remove_wakeword + add_wakeword set a new level and window size and leave the window Vec as it is; filter() drops one level per push,
    so the 56 levels stay 56 -- the gains are those of a window of 56 with the new level, NOT those of a window of 7.  (b) stream 1 is
    disconnected for chunks 40..49: gain 1 meanwhile, its window goes on afterwards from what it held -- the oracle's front-end over the
    audio without the gap.  (c) stream 2 is reset mid-run and keeps the levels of its twin, stream 3.  The oracle's detector, given the
    same remove / add_ref and (for b) not fed during the gap, reports with every detection the gain of its best window's chunk: those
    are the live gains of those chunks."""
    C0, GAP = 60, range(40, 50)
    pcm = varying_noise(4, 96, np.random.default_rng(21), silent=None)
    pcm[3] = pcm[2]
    REAL, SYN = 2, 3
    kw = dict(gain_normalizer=True, min_gain=MIN_GAIN, max_gain=MAX_GAIN)
    lv = lambda w: dicts[w]["rms_level"]
    # What the reference does, assembled from the oracle's front-end.  The window holds chunk levels only: what it contains depends on the
    # audio and on window_size, never on rms_level_ref, which enters the gain alone.  So the unshrunk window of stream 0 behind chunk 60 -- the
    # last 56 levels, one pushed and one dropped per chunk -- is the window a detector with window_size 56 holds throughout, and its gains with
    # the new level are rows C0.. of orc.frontend_stream(new level, 56).  (Every chunk of this noise has a level != 0, so the window is full
    # of 56 by chunk 55.)  orc.Detector shows a gain only with a detection, and every detection resets it for the 22 frames its window needs
    # to refill: one gain per nine chunks at best, compared further down.
    assert all(np.any(pcm[0][c * 480:(c + 1) * 480] != 0) for c in range(96))
    keep56_old = orc.frontend_stream(pcm[0], rms_level_ref=lv(REAL), window_size=56, **kw)[2]
    keep56_new = orc.frontend_stream(pcm[0], rms_level_ref=lv(SYN), window_size=56, **kw)[2]
    shrunk = orc.frontend_stream(pcm[0], rms_level_ref=lv(SYN), window_size=7, **kw)[2]
    want_a = np.concatenate([keep56_old[:C0], keep56_new[C0:]])
    assert int(np.sum(want_a[C0:] != shrunk[C0:])) >= 5, "this audio does not tell an unshrunk window from a window of 7"
    no_gap = np.concatenate([pcm[1][:GAP[0] * 480], pcm[1][(GAP[-1] + 1) * 480:]])
    g = orc.frontend_stream(no_gap, rms_level_ref=lv(SYN), window_size=7, **kw)[2]
    want_b = np.concatenate([g[:GAP[0]], np.ones(len(GAP), np.float32), g[GAP[0]:]])
    through = orc.frontend_stream(pcm[1], rms_level_ref=lv(SYN), window_size=7, **kw)[2]
    assert int(np.sum(want_b[GAP[-1] + 1:] != through[GAP[-1] + 1:])) >= 1, "the gap leaves no trace in this audio"
    want_c = orc.frontend_stream(pcm[2], rms_level_ref=lv(SYN), window_size=7, **kw)[2]
    # the live batch: every scored window reports (threshold 0, one score is enough, eager), so that the oracle's detector shows its gains
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold, cfg.min_scores, cfg.eager = 0.0, 0.0, 1, True
    sb = ra.StreamBatch(ctx, None, cfg, 4, max_chunks_per_call=2, bank=bank, stream_wakeword=[REAL, SYN, SYN, SYN], bank_filters=filters(ra, True, False))

    def act(c):
        if c == C0:
            sb.set_wakewords(0, [SYN])
            sb.reset(2)
        if c == GAP[0]:
            sb.set_wakewords(1, [-1])
        if c == GAP[-1] + 1:
            sb.set_wakewords(1, [SYN])
    got, _, rms, gains = feed(sb, pcm, (1,), before_chunk=act)
    assert np.array_equal(bits(gains[0]), bits(want_a)), np.argwhere(gains[0] != want_a).ravel()
    assert np.all(gains[1][GAP[0]:GAP[-1] + 1] == 1.0)
    assert np.array_equal(bits(gains[1]), bits(want_b)), np.argwhere(gains[1] != want_b).ravel()
    assert np.array_equal(bits(gains[2]), bits(want_c)) and np.array_equal(bits(gains[3]), bits(want_c)) and np.array_equal(bits(rms[2]), bits(rms[3]))
    assert got[2] != got[3], "the reset changed the detections of stream 2, not its levels"
    # orc.Detector with the same slot changes
    okw = dict(avg_threshold=0.0, threshold=0.0, min_scores=1, eager=True, **kw)

    def swap(d):
        d.remove(0)
        d.add_ref(dicts[SYN])
    d = orc.Detector(**okw)
    d.add_ref(dicts[REAL])
    want0 = detector_gains(d, pcm[0], {C0: swap})
    d = orc.Detector(**okw)
    d.add_ref(dicts[SYN])
    want1 = detector_gains(d, pcm[1], {GAP[0]: lambda d: d.remove(0), GAP[-1] + 1: lambda d: d.add_ref(dicts[SYN])}, skip=set(GAP))
    seen = 0
    for s, want, lens in ((0, want0, lambda c: 168 if c < C0 else 22), (1, want1, lambda c: 22)):
        assert len(got[s]) == len(want) and len(want) >= 3, (s, len(got[s]), len(want))
        for rec, (chunk, r) in zip(got[s], want):
            assert rec[0] // 3 + 1 == chunk and rec[2] == r["counter"], (s, rec, chunk, r)
            best_chunk = (rec[1] + lens(chunk) - 1) // 3 + 1
            assert gains[s][best_chunk] == r["gain"], (s, chunk, best_chunk, float(gains[s][best_chunk]), float(r["gain"]))
            seen += chunk >= C0
    assert seen >= 3, "detections behind the slot changes carry the oracle's gains"


# ---------------------------------------------------------------------------------------------- 4. one wakeword for all

@pytest.mark.parametrize("w", [1, 3])
def test_one_wakeword_for_all(ra, ctx, bank, dicts, audio, w):
    """4. Every stream indexes wakeword w: levels, gains and, under RP_ARITH_STRICT_F32, aggregates of a rp_stream_batch_new batch with
    set_filters(f, level_w); rp_frontend_batch_bank is rp_frontend_batch(f, level_w, max_len_w / 3)."""
    pcm = audio[0][10:15, :480 * 60]
    n = pcm.shape[0]
    d = dicts[w]
    level, L = d["rms_level"], bank.max_lens[w]
    f = filters(ra)
    idx = np.full(n, w, np.int32)
    a = ctx.frontend_bank(pcm, f, bank, idx)
    b = ctx.frontend(pcm, f, level, L // 3)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    assert np.mean(a[2] != 1.0) >= 0.5
    tm = ra.Templates(ctx, list(d["samples_features"].values()), d["avg_features"])
    cfg = live_config(ra)
    shared_cfg = live_config(ra)
    if d["threshold"] is not None:
        shared_cfg.threshold = d["threshold"]
    if d["avg_threshold"] is not None:
        shared_cfg.avg_threshold = d["avg_threshold"]
    A = ra.StreamBatch(ctx, None, cfg, n, max_chunks_per_call=3, bank=bank, stream_wakeword=idx, bank_filters=f)
    B = ra.StreamBatch(ctx, tm, shared_cfg, n, max_chunks_per_call=3, filters=f, rms_level_ref=level)
    before = ctx.dtw_ref_pairs()
    got_a, agg_a, rms_a, gains_a = feed(A, pcm, (3, 1, 2), want_agg=True)
    with ctx.arithmetic("strict_f32"):
        got_b, agg_b, rms_b, gains_b = feed(B, pcm, (3, 1, 2), want_agg=True)
    assert ctx.dtw_ref_pairs() == before
    assert np.array_equal(bits(rms_a), bits(rms_b)) and np.array_equal(bits(gains_a), bits(gains_b))
    assert np.array_equal(bits(gains_a), bits(a[2]))
    col = np.arange(3 + L - 1, agg_a.shape[1])   # windows that lie inside the stream
    assert len(col) > 0 and np.array_equal(bits(agg_a[:, col]), bits(agg_b[:, col]))
    assert got_a == got_b


# ---------------------------------------------------------------------------------------------- 5. device pointers

def test_device_pointer_context(ra, ctx, bank, dicts, audio):
    """5. A context without RP_CTX_HOST_POINTERS: audio, indices and outputs on the device; an index outside the bank is treated as -1.
    Test 1's first case through rp_frontend_batch_bank and the (3, 1, 2) / f32 case of test 2 through a live batch: levels, aggregates
    and detections."""
    import torch
    pcm, idx = audio
    want_det, want_agg = whole_detect(ra, ctx, bank, audio, np.float32)
    _, want_out, want_rms, want_gains = oracle_case(audio, dicts, np.float32, True)
    dctx = ra.BatchContext(device=0, host_pointers=False)
    dbank = make_bank(ra, dctx)
    bad = idx.copy()
    minus = np.flatnonzero(idx < 0)
    bad[minus[0]], bad[minus[1]] = 9, -7      # outside the bank: both streams had -1
    d_idx = torch.tensor(bad, dtype=torch.int32, device="cuda")
    d_pcm = torch.from_numpy(pcm).cuda()
    N = pcm.shape[1]
    d_out = torch.zeros((S, N), dtype=torch.float32, device="cuda")
    d_rms = torch.zeros((S, NC), dtype=torch.float32, device="cuda")
    d_gain = torch.zeros((S, NC), dtype=torch.float32, device="cuda")
    f = filters(ra)
    dctx.frontend_bank_dev(d_pcm.data_ptr(), 3, S, N, N, f, dbank, int(d_idx.data_ptr()), d_out.data_ptr(), N, d_rms.data_ptr(), d_gain.data_ptr())
    dctx.synchronize()
    assert np.array_equal(bits(d_rms.cpu().numpy()), bits(want_rms)) and np.array_equal(bits(d_gain.cpu().numpy()), bits(want_gains))
    assert np.array_equal(bits(d_out.cpu().numpy()), bits(want_out))
    sb = ra.StreamBatch(dctx, None, live_config(ra), S, max_chunks_per_call=3, bank=dbank, stream_wakeword=int(d_idx.data_ptr()), bank_filters=f)
    max_det = 8
    d_det = torch.zeros(S * max_det * 24, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(S, dtype=torch.int32, device="cuda")
    L = ra.load_library()
    c, k, rows, aggs, got = 0, 0, [], [], [[] for _ in range(S)]
    while c < NC:
        n = min((3, 1, 2)[k % 3], NC - c)
        k += 1
        part = d_pcm[:, c * 480:(c + n) * 480].contiguous()
        d_agg = torch.zeros((S, 3 * n), dtype=torch.float32, device="cuda")
        sb.process_dev(part.data_ptr(), 3, n, n * 480, d_det.data_ptr(), d_n.data_ptr(), max_det, d_agg.data_ptr())
        lr = torch.zeros((S, n), dtype=torch.float32, device="cuda")
        lg = torch.zeros((S, n), dtype=torch.float32, device="cuda")
        assert L.rp_stream_batch_levels(sb._h, C.c_void_p(lr.data_ptr()), C.c_void_p(lg.data_ptr())) == 0
        dctx.synchronize()
        rows.append((lr.cpu().numpy(), lg.cpu().numpy()))
        aggs.append(d_agg.cpu().numpy())
        det = np.frombuffer(d_det.cpu().numpy().tobytes(), dtype=ra.api.DET_DTYPE).reshape(S, max_det)
        nd = d_n.cpu().numpy()
        for s in range(S):
            assert nd[s] <= max_det
            for d in det[s][:nd[s]]:
                got[s].append((int(d["frame"]), int(d["window"]), int(d["counter"]), bits1(d["score"]), bits1(d["avg_score"])))
        c += n
    assert np.array_equal(bits(np.concatenate([r for r, _ in rows], axis=1)), bits(want_rms))
    assert np.array_equal(bits(np.concatenate([g for _, g in rows], axis=1)), bits(want_gains))
    assert dctx.dtw_ref_pairs() == 0
    assert same_aggregates(dbank, idx, np.concatenate(aggs, axis=1), want_agg) > 0   # (idx: the two indices outside the bank count as -1)
    assert got == want_det


# ---------------------------------------------------------------------------------------------- 6. edges and refusals

@pytest.mark.parametrize("n_streams", [1, 63, 64, 65])
def test_stream_counts_and_a_short_tail(ra, ctx, bank, dicts, audio, n_streams):
    """6. S around one wave, n_samples with a tail shorter than a chunk (never framed: copied), max_chunks_per_call 1"""
    pcm, idx = audio
    n = 480 * 20 + 123
    x, ix = np.ascontiguousarray(pcm[:n_streams, :n]), idx[:n_streams]
    if n_streams > 13:
        x[13] = 0   # silence on a stream with a wakeword: a level of 0 does not enter the window
        assert ix[13] == 2
    _, want_rms, want_gains = oracle_rows(x[:, :480 * 20], ix, dicts, True)
    want_out = oracle_rows(x, ix, dicts, True)[0]
    out, rms, gains = ctx.frontend_bank(x, filters(ra), bank, ix)
    assert rms.shape == (n_streams, 20)
    assert np.array_equal(bits(rms), bits(want_rms)) and np.array_equal(bits(gains), bits(want_gains)) and np.array_equal(bits(out), bits(want_out))
    assert np.array_equal(out[:, 480 * 20:], x[:, 480 * 20:])
    sb = ra.StreamBatch(ctx, None, live_config(ra), n_streams, max_chunks_per_call=1, bank=bank, stream_wakeword=ix, bank_filters=filters(ra))
    _, _, lr, lg = feed(sb, x[:, :480 * 20], (1,))
    assert np.array_equal(bits(lr), bits(want_rms)) and np.array_equal(bits(lg), bits(want_gains))


def test_no_wakewords_at_all(ra, ctx, bank, audio):
    """6. An empty bank and all indices -1: gains of 1, the samples pass the gain stage unchanged (the band-pass still runs), no detection"""
    pcm = audio[0][:5, :480 * 12]
    f = filters(ra)
    want = [orc.frontend_stream(pcm[s], band_pass=True, low_cutoff=LOW, high_cutoff=HIGH) for s in range(5)]
    empty = ra.WakewordBank(ctx, wakewords=[])
    assert empty.rms_levels.shape == (0,)
    empty.set_rms_levels([])
    for bk in (empty, bank):
        idx = np.full(5, -1, np.int32)
        out, rms, gains = ctx.frontend_bank(pcm, f, bk, idx)
        assert np.all(gains == 1.0)
        for s in range(5):
            assert np.array_equal(bits(out[s]), bits(want[s][0])) and np.array_equal(bits(rms[s]), bits(want[s][1]))
        sb = ra.StreamBatch(ctx, None, live_config(ra), 5, max_chunks_per_call=4, bank=bk, stream_wakeword=idx, bank_filters=f)
        got, _, lr, lg = feed(sb, pcm, (4,))
        assert not any(got) and np.all(lg == 1.0) and np.array_equal(bits(lr), bits(rms))


def test_set_rms_levels(ra, ctx, dicts, audio):
    """6. rp_wakeword_bank_set_rms_levels: the next call works with the new levels; a bank of rp_wakeword_bank_new starts without any"""
    pcm = audio[0][:3, :480 * 30]
    d = dicts[3]
    plain = ra.WakewordBank(ctx, wakewords=[(list(d["samples_features"].values()), None, None, None)] * 2)
    assert np.all(np.isnan(plain.rms_levels))
    idx = np.array([0, 1, 0], np.int32)
    f = filters(ra, True, False)
    assert np.all(ctx.frontend_bank(pcm, f, plain, idx)[2] == 1.0)
    sb = ra.StreamBatch(ctx, None, live_config(ra), 3, max_chunks_per_call=2, bank=plain, stream_wakeword=idx, bank_filters=f)
    assert np.all(feed(sb, pcm[:, :480 * 4], (2,))[3] == 1.0)
    plain.set_rms_levels([0.05, float("nan")])
    assert plain.rms_levels[0] == np.float32(0.05) and np.isnan(plain.rms_levels[1])
    gains = ctx.frontend_bank(pcm, f, plain, idx)[2]
    want = orc.frontend_stream(pcm[0], gain_normalizer=True, min_gain=MIN_GAIN, max_gain=MAX_GAIN, rms_level_ref=0.05, window_size=7)[2]
    assert np.array_equal(bits(gains[0]), bits(want)) and np.all(gains[1] == 1.0) and np.mean(want != 1.0) >= 0.5
    # the live batch made before the change reads the new levels from its next call on: its window was empty until now
    live = feed(sb, pcm[:, 480 * 4:], (2,))[3]
    want_live = orc.frontend_stream(pcm[0][480 * 4:], gain_normalizer=True, min_gain=MIN_GAIN, max_gain=MAX_GAIN, rms_level_ref=0.05, window_size=7)[2]
    assert np.array_equal(bits(live[0]), bits(want_live)) and np.all(live[1] == 1.0)
    L = ra.load_library()
    assert np.isnan(L.rp_wakeword_bank_rms_level(plain._h, 2)) and np.isnan(L.rp_wakeword_bank_rms_level(plain._h, -1))
    assert np.isnan(L.rp_wakeword_bank_rms_level(None, 0))
    assert L.rp_wakeword_bank_set_rms_levels(plain._h, None) == -1 and b"null argument" in L.rp_last_error()
    assert L.rp_wakeword_bank_set_rms_levels(None, None) == -1 and b"null handle" in L.rp_last_error()
    with pytest.raises(ValueError):
        plain.set_rms_levels([0.05])


def test_refusals_leave_the_batch_as_it_was(ra, ctx, bank, dicts, audio):
    """6. set_filters_bank on a batch that is not over a bank, after audio, with 22.05 kHz input in either order: each is refused with a
    message and the batch goes on like a twin that never saw the call; an out-of-range host index fails rp_frontend_batch_bank before
    anything is written."""
    pcm = np.ascontiguousarray(audio[0][20:25, :480 * 12])
    f = filters(ra)
    cfg = live_config(ra)
    idx = [0, 3, -1, 5, 8]

    def same_run(a, b, x):
        ra_, rb = feed(a, x, (2, 1), want_agg=True), feed(b, x, (2, 1), want_agg=True)
        assert ra_[0] == rb[0] and np.array_equal(bits(ra_[1]), bits(rb[1])) and np.array_equal(bits(ra_[2]), bits(rb[2])) and np.array_equal(bits(ra_[3]), bits(rb[3]))

    d = dicts[3]
    tm = ra.Templates(ctx, list(d["samples_features"].values()))
    a = ra.StreamBatch(ctx, tm, cfg, 5, max_chunks_per_call=2, filters=f, rms_level_ref=0.05)
    twin = ra.StreamBatch(ctx, tm, cfg, 5, max_chunks_per_call=2, filters=f, rms_level_ref=0.05)
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_filters_bank: the batch was not made by rp_stream_batch_new_bank"):
        a.set_filters_bank(f)
    same_run(a, twin, pcm)
    # after the first audio
    a = ra.StreamBatch(ctx, None, cfg, 5, max_chunks_per_call=2, bank=bank, stream_wakeword=idx, bank_filters=f)
    twin = ra.StreamBatch(ctx, None, cfg, 5, max_chunks_per_call=2, bank=bank, stream_wakeword=idx, bank_filters=f)
    a.process(pcm[:, :480]); twin.process(pcm[:, :480])
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_filters_bank: the streams have already received audio"):
        a.set_filters_bank(filters(ra, True, False))
    same_run(a, twin, pcm[:, 480:])
    # filters, then 22.05 kHz input
    a = ra.StreamBatch(ctx, None, cfg, 5, max_chunks_per_call=2, bank=bank, stream_wakeword=idx, bank_filters=f)
    twin = ra.StreamBatch(ctx, None, cfg, 5, max_chunks_per_call=2, bank=bank, stream_wakeword=idx, bank_filters=f)
    with pytest.raises(ra.RustpotterError, match="40 ms"):
        a.set_input(22050)
    assert a.samples_per_chunk == 480
    same_run(a, twin, pcm)
    # 22.05 kHz input, then filters
    a = ra.StreamBatch(ctx, None, cfg, 5, max_chunks_per_call=2, sample_rate=22050, bank=bank, stream_wakeword=idx)
    twin = ra.StreamBatch(ctx, None, cfg, 5, max_chunks_per_call=2, sample_rate=22050, bank=bank, stream_wakeword=idx)
    with pytest.raises(ra.RustpotterError, match="40 ms"):
        a.set_filters_bank(f)
    assert a.samples_per_chunk == 882
    x = np.ascontiguousarray(audio[0][20:25, :882 * 2])
    for sb in (a, twin):
        with pytest.raises(ra.RustpotterError):
            sb.levels()
    ra_, rb = a.process(x, want_agg=True), twin.process(x, want_agg=True)
    assert np.array_equal(ra_[1], rb[1]) and np.array_equal(bits(ra_[2]), bits(rb[2]))
    # the old call still refuses the gain normaliser on a bank batch, and names the new one
    a = ra.StreamBatch(ctx, None, cfg, 5, max_chunks_per_call=2, bank=bank, stream_wakeword=idx)
    with pytest.raises(ra.RustpotterError, match="gain normaliser is not available on a batch over a wakeword bank.*rp_stream_batch_set_filters_bank"):
        a.set_filters(f, 0.05)
    # the band-pass alone through the new call is the old call
    bp = filters(ra, False, True)
    a = ra.StreamBatch(ctx, None, cfg, 5, max_chunks_per_call=2, bank=bank, stream_wakeword=idx, bank_filters=bp)
    twin = ra.StreamBatch(ctx, None, cfg, 5, max_chunks_per_call=2, bank=bank, stream_wakeword=idx, filters=bp)
    same_run(a, twin, pcm)
    # the gain normaliser off: gains of 1, everything else what rp_frontend_batch gives with the band-pass alone
    o1, r1, g1 = ctx.frontend_bank(pcm, bp, bank, np.array(idx, np.int32))
    o2, r2, g2 = ctx.frontend(pcm, bp, 0.05, 7)
    assert np.all(g1 == 1.0) and np.all(g2 == 1.0) and np.array_equal(bits(o1), bits(o2)) and np.array_equal(bits(r1), bits(r2))
    # an index outside the bank in a host array
    out = np.full((5, pcm.shape[1]), 7.0, np.float32)
    rms = np.full((5, 12), 7.0, np.float32)
    gains = np.full((5, 12), 7.0, np.float32)
    bad = np.array([0, 1, 9, 2, 3], np.int32)
    L = ra.load_library()
    fc = ra.RustpotterConfig()
    fc.filters = f
    cf = fc._filters_c()
    r = L.rp_frontend_batch_bank(ctx._h, pcm.ctypes.data, 3, 5, pcm.shape[1], pcm.shape[1], C.byref(cf), bank._h, bad.ctypes.data, out.ctypes.data,
                                 pcm.shape[1], rms.ctypes.data, gains.ctypes.data)
    assert r == -1 and b"stream 2: wakeword index 9 is outside the bank (-1 .. 8)" in L.rp_last_error()
    assert np.all(out == 7.0) and np.all(rms == 7.0) and np.all(gains == 7.0)
    other = ra.BatchContext(device=0, host_pointers=True)
    with pytest.raises(ra.RustpotterError, match="the bank belongs to another context"):
        other.frontend_bank(pcm, f, bank, bad)
