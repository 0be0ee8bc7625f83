"""A wakeword bank that changes (rp_wakeword_bank_reserve / _put / _put_from_rpw / _enrol; bank_put_kernel, bank_move_kernel), also under
live-stream batches.  No tolerance anywhere: every check is bit equality (float arrays compared as uint32, exact detection records) between
the new path and an entry point that existed before it -- rp_wakeword_bank_new / _new_from_rpw, rp_wakeword_ref_build_batch -- which the
other bank tests tie to the oracle."""
import os

import numpy as np
import pytest

import rpw_py
import simstream
from oracle import rp_oracle as orc

pytestmark = pytest.mark.gpu

G = simstream.GOLDEN
SEED = 0x5EED00000BA2C0DE
COUNTS = [1, 2, 5, 32]
LENS = [1, 2, 63, 64, 65, 70]
GOLDEN_SETS = [
    ("oye casa", ["oye_casa_g_%d.wav" % i for i in range(1, 6)], 0.5, None),
    ("oye casa real", ["oye_casa_real_%d.wav" % i for i in range(1, 7)], None, None),
    ("alexa", ["alexa.wav", "alexa2.wav", "alexa3.wav"], None, 0.2),
]


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


def modes(ra):
    return [ra.ScoreMode.Max, ra.ScoreMode.Average, ra.ScoreMode.Median]


# ------------------------------------------------------------------------------------------------------------------ synthetic wakewords

_SYNTH = {}


def synth(K):
    """12 wakewords: template counts from {1, 2, 5, 32}, lengths from {1, 2, 63, 64, 65, 70}, an averaged template of the first sample's
    length on some, own thresholds on some; and 12 streams of 80 random frames"""
    if K not in _SYNTH:
        rng = np.random.default_rng(1000 + K)
        ww = []
        for w in range(12):
            T = COUNTS[w % 4] if w < 8 else int(rng.choice(COUNTS))
            lens = [int(x) for x in rng.choice(LENS, T)]
            if w < len(LENS):
                lens[0] = LENS[w]   # every length heads a wakeword at least once
            tm = [orc.synth_templates(SEED + 1000 * K + 40 * w + t, 1, L, K)[0] for t, L in enumerate(lens)]
            avg = orc.synth_templates(SEED + 1000 * K + 40 * w + 39, 1, lens[0], K)[0] if w % 3 != 1 else None
            ww.append((tm, avg, 0.4 if w % 4 == 0 else None, 0.1 if w % 5 == 0 else None))
        mfcc = rng.standard_normal((12, 80, K)).astype(np.float32)
        _SYNTH[K] = (ww, mfcc)
    return _SYNTH[K]


def other(K, n, lens_of=lambda i: [70, 3]):
    """further wakewords, not among synth(K)'s"""
    out = []
    for i in range(n):
        lens = lens_of(i)
        tm = [np.array(orc.synth_templates(SEED + 777000 + 1000 * K + 40 * i + t, 1, L, K)[0], np.float32) for t, L in enumerate(lens)]
        out.append((tm, tm[0] * np.float32(0.5), None, None))
    return out


def score_all(ra, ctx, bank, mfcc, idx):
    """rp_dtw_score_bank in the three score modes, without and with the averaged templates -> a list of (avg bits or None, agg bits)"""
    out = []
    for mode in modes(ra):
        for with_avg in (False, True):
            avg, agg = ctx.dtw_scores_bank(mfcc, bank, idx, score_mode=mode, with_avg=with_avg, win_pitch=80)
            out.append((None if avg is None else bits(avg).copy(), bits(agg).copy()))
    return out


def same_scores(a, b, rows=None):
    for (avg_a, agg_a), (avg_b, agg_b) in zip(a, b):
        sel = slice(None) if rows is None else rows
        assert np.array_equal(agg_a[sel], agg_b[sel])
        assert (avg_a is None) == (avg_b is None)
        if avg_a is not None:
            assert np.array_equal(avg_a[sel], avg_b[sel])


def grown_bank(ra, ctx, K):
    """bank B of the issue: the first 2 wakewords at creation, the other 10 put in calls of 3 + 3 + 4 without any reserve"""
    ww, _ = synth(K)
    b = ra.WakewordBank(ctx, wakewords=ww[:2])
    assert b.pool_growths == 0
    b.put(2, ww[2:5])
    b.put(5, ww[5:8])
    b.put(8, ww[8:12])
    return b


@pytest.mark.parametrize("K", [5, 16])
def test_put_equals_create(ra, ctx, K):
    """1. A bank put together piece by piece scores bit for bit as the bank made in one piece; its pools (created exactly full) grew."""
    ww, mfcc = synth(K)
    a = ra.WakewordBank(ctx, wakewords=ww)
    b = grown_bank(ra, ctx, K)
    assert b.pool_growths >= 1, "pools created exactly full cannot take ten more wakewords without growing"
    assert b.W == 12 and ctx._L.rp_wakeword_bank_size(b._h) == 12 and b.reserved_len == 0
    assert b.max_lens == a.max_lens and b.max_len == a.max_len
    assert np.array_equal(bits(a.rms_levels), bits(b.rms_levels))   # NaN for all
    idx = np.arange(12, dtype=np.int32)
    same_scores(score_all(ra, ctx, a, mfcc, idx), score_all(ra, ctx, b, mfcc, idx))
    b.put(12, [])   # n == 0 succeeds and changes nothing
    assert b.W == 12


@pytest.mark.parametrize("K", [5, 16])
def test_special_rows(ra, ctx, K):
    """2. Rows the host loop treats specially: all zero (stays zero, exempt from the norm range), squared norm below kDtwNormLo and above
    kDtwNormHiRow (the wakeword takes the reference-shaped cell).  Same bits and the same number of rescored pairs as the bank made on the host."""
    rng = np.random.default_rng(7 + K)
    ww = other(K, 4, lambda i: [20, 12 + i])
    ww[0][0][1][5, :] = 0.0
    ww[1][0][0][3, :] = 1e-20
    ww[2][0][1][0, :] = 1e10
    ww[3][1][7, :] = 1e-20   # in an averaged template
    mfcc = rng.standard_normal((4, 80, K)).astype(np.float32)
    idx = np.arange(4, dtype=np.int32)
    a = ra.WakewordBank(ctx, wakewords=ww)
    b = ra.WakewordBank(ctx, wakewords=[], mfcc_size=K)
    b.put(0, ww[:1])
    b.put(1, ww[1:])
    for mode in modes(ra):
        n0 = ctx.dtw_ref_pairs()
        avg_a, agg_a = ctx.dtw_scores_bank(mfcc, a, idx, score_mode=mode, with_avg=True, win_pitch=80)
        n1 = ctx.dtw_ref_pairs()
        avg_b, agg_b = ctx.dtw_scores_bank(mfcc, b, idx, score_mode=mode, with_avg=True, win_pitch=80)
        n2 = ctx.dtw_ref_pairs()
        assert np.array_equal(bits(agg_a), bits(agg_b)) and np.array_equal(bits(avg_a), bits(avg_b))
        print("pairs rescored with the reference-shaped cell: %d (host-made bank), %d (put)" % (n1 - n0, n2 - n1))
        assert n1 - n0 == n2 - n1 and n1 - n0 > 0


@pytest.mark.parametrize("K", [5, 16])
def test_replace(ra, ctx, K):
    """3. A wakeword put over index 3, twice (garbage accumulates), then enough further wakewords for one more growth (which drops the
    garbage): index 3 scores as the new wakeword in a fresh bank, every other index as before."""
    ww, mfcc = synth(K)
    b = grown_bank(ra, ctx, K)
    idx = np.arange(12, dtype=np.int32)
    before = score_all(ra, ctx, b, mfcc, idx)
    first, second = other(K, 2, lambda i: [66 + i, 9, 70])
    b.put(3, [first])
    b.put(3, [second])
    assert b.W == 12 and b.max_lens[3] == 70
    grown = b.pool_growths
    more = other(K, 12, lambda i: [30 + i] * 5)[2:]
    at = 12
    while b.pool_growths == grown:
        assert at < 12 + len(more), "ten more wakewords of five templates must outgrow the pools"
        b.put(at, [more[at - 12]])
        at += 1
    assert b.W == at
    after = score_all(ra, ctx, b, mfcc, idx)
    keep = np.array([w for w in range(12) if w != 3])
    same_scores(before, after, rows=keep)
    fresh = ra.WakewordBank(ctx, wakewords=[second])
    same_scores([(None if avg is None else avg[3:4], agg[3:4]) for avg, agg in after],
                score_all(ra, ctx, fresh, mfcc[3:4], np.zeros(1, np.int32)))
    # the appended ones score as in a bank of their own too
    tail = ra.WakewordBank(ctx, wakewords=more[:at - 12])
    n = at - 12
    same_scores(score_all(ra, ctx, b, mfcc[:n], np.arange(12, at, dtype=np.int32)), score_all(ra, ctx, tail, mfcc[:n], np.arange(n, dtype=np.int32)))


# -------------------------------------------------------------------------------------------------------------------- golden recordings

def golden_wakewords():
    return [(name, {w: read(w) for w in wavs}, thr, athr) for name, wavs, thr, athr in GOLDEN_SETS]


@pytest.fixture(scope="module")
def golden_rpw(ctx):
    """the three golden recording sets at mfcc_size 16 through rp_wakeword_ref_build_batch: the yardstick of the enrolment tests"""
    return ctx.build_wakeword_refs(golden_wakewords(), 16)


def recording(name):
    """a golden recording as 16 kHz f32 (the 48 kHz ones through the oracle's resampler)"""
    a, sr, ch = rpw_py.read_wav(os.path.join(G, name))
    assert ch == 1
    if a.dtype == np.int16:
        a = simstream.i16_to_f32(a)
    if sr != 16000:
        a = orc.resample_stream(a, sr)
    return np.ascontiguousarray(a, np.float32)


def padded(rng, rec, n):
    """0.3 s of noise, the recording, noise up to n samples ('silence' that is not digital zero)"""
    return np.concatenate([noise(rng, 4800), rec, noise(rng, n - 4800 - len(rec))])


def noise(rng, n):
    return (1e-3 * rng.standard_normal(n)).astype(np.float32)


@pytest.fixture(scope="module")
def golden_pcm():
    """six streams of one length (a multiple of 480): the first recording of each golden set twice over, then two of noise"""
    rng = np.random.default_rng(77)
    recs = [recording(n) for n in ("oye_casa_g_1.wav", "oye_casa_real_1.wav", "alexa.wav")]
    n = 480 * ((4800 + max(len(r) for r in recs) + 24000 + 479) // 480)
    rows = [padded(rng, recs[0], n), padded(rng, recs[1], n), padded(rng, recs[2], n), padded(rng, recs[0], n),
            (0.1 * rng.standard_normal(n)).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32)]
    return np.stack(rows), np.array([0, 1, 2, 0, 1, 2], np.int32), recs


def detect_all(ctx, bank, pcm, idx, cfg):
    det, n_det, agg, avg = ctx.batch_detect_bank(pcm, bank, idx, cfg, max_det=16, want_agg=True)
    return det.tobytes(), n_det.tolist(), bits(agg).copy(), bits(avg).copy()


@pytest.mark.parametrize("want_rpw", [True, False])
def test_enrol_equals_build_and_load(ra, ctx, golden_rpw, golden_pcm, want_rpw):
    """4. rp_wakeword_bank_enrol into an empty bank against rp_wakeword_ref_build_batch -> rp_wakeword_bank_new_from_rpw: the same .rpw
    bytes (when asked for), the same rms levels, the same detections and scores over the golden recordings."""
    pcm, idx, _ = golden_pcm
    want = ra.WakewordBank(ctx, rpw=golden_rpw)
    got = ra.WakewordBank(ctx, wakewords=[], mfcc_size=16)
    out = got.enrol(0, golden_wakewords(), want_rpw=want_rpw)
    if want_rpw:
        assert out == golden_rpw
    else:
        assert out is None
    assert got.W == 3 and got.max_lens == want.max_lens and got.max_len == want.max_len
    assert np.array_equal(bits(got.rms_levels), bits(want.rms_levels)) and not np.isnan(got.rms_levels).any()
    for mode in modes(ra):
        cfg = ra.DetectorConfig()
        cfg.score_mode = mode
        a, b = detect_all(ctx, want, pcm, idx, cfg), detect_all(ctx, got, pcm, idx, cfg)
        assert a[1] == b[1] and a[0] == b[0]
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        if mode == ra.ScoreMode.Max:
            print("detections per stream:", a[1])
            assert sum(a[1][:4]) >= 1 and a[1][4:] == [0, 0]


def records(det, n_det):
    """per stream the exact detection records of a process call, without the stream's bank index"""
    return [[(int(d["frame"]), int(d["window"]), int(d["counter"]), int(np.float32(d["score"]).view(np.uint32)),
              int(np.float32(d["avg_score"]).view(np.uint32))) for d in det[s][:n_det[s]]] for s in range(len(n_det))]


class Pair:
    """a live batch and its control, driven by the same calls"""

    def __init__(self, ra, ctx, banks, S, filters):
        cfg = ra.DetectorConfig()
        self.sb = [ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=4, bank=b, stream_wakeword=[-1] * S, bank_filters=filters) for b in banks]
        self.filters = filters is not None
        self.n = 0

    def feed(self, pcm, chunks_per_call):
        for c in range(0, pcm.shape[1] // 480, chunks_per_call):
            part = np.ascontiguousarray(pcm[:, c * 480:(c + chunks_per_call) * 480])
            res = [sb.process(part, max_det=4, want_agg=True) for sb in self.sb]
            assert records(res[0][0], res[0][1]) == records(res[1][0], res[1][1])
            assert np.array_equal(bits(res[0][2]), bits(res[1][2]))
            if self.filters:
                lv = [sb.levels() for sb in self.sb]
                assert np.array_equal(bits(lv[0][0]), bits(lv[1][0])) and np.array_equal(bits(lv[0][1]), bits(lv[1][1]))
            self.n += int(res[0][1].sum())

    def close(self):
        for sb in self.sb:
            sb.close()


@pytest.mark.parametrize("filtered", [False, True])
def test_live_growth(ra, ctx, golden_rpw, golden_pcm, filtered):
    """5. A service's first day: an empty reserved bank, a live batch over it, wakewords enrolled and replaced while the batch runs.  The
    control is a batch over a bank that held everything from the start, driven by the same calls: detections and the aggregate of every
    call are the same bits (and, with the per-stream gain normaliser and the band-pass, so are the levels and gains)."""
    _, _, recs = golden_pcm
    rng = np.random.default_rng(5)
    S = 5
    filters = None
    if filtered:
        filters = ra.FiltersConfig()
        filters.gain_normalizer.enabled, filters.gain_normalizer.min_gain, filters.gain_normalizer.max_gain = True, 0.2, 4.0
        filters.band_pass.enabled, filters.band_pass.low_cutoff, filters.band_pass.high_cutoff = True, 80.0, 500.0
    live = ra.WakewordBank(ctx, wakewords=[], mfcc_size=16)
    live.reserve(max_len=200)
    assert live.reserved_len == 200 and live.W == 0 and live.max_len == 0
    control = ra.WakewordBank(ctx, rpw=golden_rpw)
    control.reserve(max_len=200)
    p = Pair(ra, ctx, [live, control], S, filters)
    p.feed(0.1 * rng.standard_normal((S, 10 * 480)).astype(np.float32), 2)
    assert p.n == 0
    # two wakewords arrive; streams 1 and 3 connect
    live.enrol(0, golden_wakewords()[:2])
    assert live.W == 2 and live.max_lens == control.max_lens[:2]
    for sb in p.sb:
        sb.set_wakewords(1, [0])
        sb.set_wakewords(3, [1])
    n = 480 * ((4800 + max(len(recs[0]), len(recs[1])) + 24000 + 479) // 480)
    pcm = np.stack([noise(rng, n), padded(rng, recs[0], n), noise(rng, n), padded(rng, recs[1], n), noise(rng, n)])
    p.feed(pcm, 1)
    first = p.n
    print("detections after the enrolment:", first)
    assert first >= 1, "no detection: the comparison shows nothing"
    # the wakeword at index 0 is replaced while stream 1 holds it; the control has the new one at index 2
    live.put_rpw(0, golden_rpw[2:3])
    assert live.W == 2 and live.max_lens[0] == control.max_lens[2]
    p.sb[0].set_wakewords(1, [0])
    p.sb[1].set_wakewords(1, [2])
    n = 480 * ((4800 + len(recs[2]) + 24000 + 479) // 480)
    pcm = np.stack([noise(rng, n), padded(rng, recs[2], n), noise(rng, n), noise(rng, n), noise(rng, n)])
    p.feed(pcm, 1)
    print("detections after the replacement:", p.n - first)
    assert p.n > first, "the replaced wakeword never fired"
    p.close()


def test_ceiling_changes_no_bits(ra, ctx, golden_rpw, golden_pcm):
    """6. The same bank and audio through a batch over the bank reserved to 200 frames and a batch over it unreserved: a longer history
    changes no detection and no aggregate (compared from the first window that lies within the stream)."""
    pcm, idx, _ = golden_pcm
    banks = [ra.WakewordBank(ctx, rpw=golden_rpw), ra.WakewordBank(ctx, rpw=golden_rpw)]
    banks[0].reserve(max_len=200)
    cfg = ra.DetectorConfig()
    out = []
    for b in banks:
        sb = ra.StreamBatch(ctx, None, cfg, len(idx), max_chunks_per_call=8, bank=b, stream_wakeword=idx)
        dets, aggs = [], []
        for c in range(0, pcm.shape[1] // 480, 8):
            det, n_det, agg = sb.process(np.ascontiguousarray(pcm[:, c * 480:(c + 8) * 480]), max_det=8, want_agg=True)
            dets.append(records(det, n_det))
            aggs.append(agg)
        out.append((dets, np.concatenate(aggs, axis=1)))
        sb.close()
    assert out[0][0] == out[1][0] and sum(len(d) for call in out[0][0] for d in call) >= 1
    for s, w in enumerate(idx):
        f0 = banks[0].max_lens[w] - 1 + 3   # column j of the live rows is frame j - 3
        assert np.array_equal(bits(out[0][1][s, f0:]), bits(out[1][1][s, f0:])), s


# ----------------------------------------------------------------------------------------------------------------------------- refusals

def state(ra, ctx, bank, mfcc):
    idx = np.arange(bank.W, dtype=np.int32) % max(bank.W, 1)
    avg, agg = ctx.dtw_scores_bank(mfcc[:bank.W], bank, idx, with_avg=True, win_pitch=80)
    return (ctx._L.rp_wakeword_bank_size(bank._h), ctx._L.rp_wakeword_bank_max_len(bank._h, -1), bank.reserved_len, bits(bank.rms_levels).tobytes(),
            bits(avg).tobytes(), bits(agg).tobytes())


def test_refusals_leave_the_bank_as_it_was(ra, ctx, golden_rpw):
    """7. Every refused call leaves size, longest window, rms levels and the scores of a probe call unchanged."""
    K = 16
    ww, mfcc = synth(K)
    bank = ra.WakewordBank(ctx, wakewords=ww[:4])
    bank.set_rms_levels([0.1, 0.2, float("nan"), 0.4])
    was = state(ra, ctx, bank, mfcc)
    good = other(K, 3, lambda i: [10, 20])

    def refused(match, call):
        with pytest.raises(ra.RustpotterError, match=match):
            call()
        assert state(ra, ctx, bank, mfcc) == was, match

    bad = other(K, 1, lambda i: [10, 20])[0]
    bad[0][1][7, 3] = np.inf
    refused("wakeword 5: template features must be finite", lambda: bank.put(4, [good[0], bad, good[1]]))   # ... and the first one is not added
    refused("wakeword 2: template features must be finite", lambda: bank.put(2, [bad]))
    nan_avg = (good[0][0], np.full((10, K), np.nan, np.float32), None, None)
    refused("wakeword 4: template features must be finite", lambda: bank.put(4, [nan_avg]))
    refused("first wakeword index 5 is past the bank's 4 wakewords", lambda: bank.put(5, good[:1]))
    refused("wakeword 4: 33 templates; a bank takes at most 32", lambda: bank.put(4, other(K, 1, lambda i: [4] * 33)))
    long_avg = (good[0][0], np.ones((21, K), np.float32), None, None)
    refused("wakeword 1: averaged template of 21 frames is longer than the longest sample template", lambda: bank.put(1, [long_avg]))
    refused("wakeword 4: Usage of wakewords with different mfcc size is not supported", lambda: bank.put_rpw(4, [read("alexa.rpw")]))
    refused("wakeword 5: a wakeword model cannot be part of a bank", lambda: bank.put_rpw(4, [golden_rpw[0], read("ok_casa-tiny.rpw")]))
    refused("wakeword 4: wakeword template of 3000 frames is too long for the device kernels", lambda: bank.put(4, other(K, 1, lambda i: [3000])))
    L = ctx._L
    assert L.rp_wakeword_bank_put(None, 0, 1, None, None, None, None, None, None, None, None) == -1 and L.rp_wakeword_bank_reserve(None, 80, 0, 0) == -1
    assert L.rp_wakeword_bank_put_from_rpw(None, 0, 1, None, None) == -1 and L.rp_wakeword_bank_size(None) == -1
    assert L.rp_wakeword_bank_enrol(None, 0, 1, None, None, None, None, None, None, None, 1, None, None) == -1
    assert state(ra, ctx, bank, mfcc) == was
    refused("max_len 69 is below the bank's longest wakeword", lambda: bank.reserve(max_len=69))
    # a live batch and no reserved length: nothing longer than the current longest (70 frames) gets in
    longer = other(K, 1, lambda i: [71])
    sb = ra.StreamBatch(ctx, None, ra.DetectorConfig(), 2, bank=bank, stream_wakeword=[0, -1])
    refused("wakeword 4: window of 71 frames is longer than the bank's longest \\(70 frames\\) while a stream batch runs over the bank: "
            "call rp_wakeword_bank_reserve before creating the batch", lambda: bank.put(4, longer))
    refused("the reserved length can only change while no stream batch runs over the bank", lambda: bank.reserve(max_len=100))
    sb.close()
    bank.put(4, longer)
    assert bank.W == 5 and bank.max_len == 71
    bank.put(4, good[:1])   # replaced by a shorter one: the longest is 70 again
    assert bank.W == 5 and bank.max_len == 70
    bank.reserve(max_len=80)
    was = state(ra, ctx, bank, mfcc)
    refused("wakeword 5: window of 81 frames is longer than the bank's reserved length \\(80 frames", lambda: bank.put(5, other(K, 1, lambda i: [81])))
    sb = ra.StreamBatch(ctx, None, ra.DetectorConfig(), 2, bank=bank, stream_wakeword=[0, -1])
    refused("the reserved length can only change while no stream batch runs over the bank", lambda: bank.reserve(max_len=100))
    bank.put(5, other(K, 1, lambda i: [80]))   # up to the reserved length it goes, batch or not
    assert bank.W == 6 and bank.max_len == 80
    sb.close()
    bank.reserve(max_len=100)   # ... and may be raised again once the batch is gone
    assert bank.reserved_len == 100


def test_reserved_empty_bank_declares_its_size(ra, ctx):
    """A reserved bank without wakewords: its (mfcc_size, band_size) pair is checked although it is empty; unreserved it is a Rustpotter
    without wakewords, as before."""
    cfg = ra.DetectorConfig()
    cfg.band_size = 9
    bank = ra.WakewordBank(ctx, wakewords=[], mfcc_size=16)
    ra.StreamBatch(ctx, None, cfg, 2, bank=bank, stream_wakeword=[-1, -1]).close()
    bank.reserve(max_len=50)
    with pytest.raises(ra.RustpotterError, match="mfcc_size 16 with band_size 9 is not built"):
        ra.StreamBatch(ctx, None, cfg, 2, bank=bank, stream_wakeword=[-1, -1])
