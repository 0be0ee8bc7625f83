"""The gain normaliser where a stream holds several entries of a bank, or a model: wakeword sets, model banks and model sets.  A Rustpotter with
several wakewords works towards the largest non-NaN rms_level of its wakewords over a window of max_mfcc_frames / 3 chunk levels
(on_wakeword_change, src/detector.rs:328-338); gain_targets_kernel prepares that level and window per stream in front of the per-stream gain
kernels: rp_frontend_batch_bank_sets / rp_frontend_batch_model_bank over whole recordings, rp_stream_batch_set_filters_per_stream on live
batches, with rp_model_bank_set_rms_levels / rp_model_bank_rms_level.  Checked bit for bit against the CPU oracle's front-end per stream with
target(s) and Lmax(s) // 3, live against whole, against the oracle's chunk-wise detector (add_ref x n / add_model x n), across retargeting and
bank updates, and against the one-wakeword calls for sets of one.  The wakeword bank, its audio generator and the feeding helpers are those of
tests/test_gpu_bank_filters.py."""
import ctypes as C
import os

import numpy as np
import pytest

import rpw_py
import simstream
from oracle import rp_oracle as orc
from test_gpu_bank_filters import GOLDEN_RPW, NAN_W, WINDOWS, as_format, bits, bits1, feed, make_bank, synth_dicts, utterances, varying_noise

pytestmark = pytest.mark.gpu

G = simstream.GOLDEN
S, NC = 130, 90                      # two full workgroups of the preparation kernel and a partial one; the 56-window wraps in 90 chunks
MIN_GAIN, MAX_GAIN = 0.3, 2.0        # both are reached by noise of 0.01 .. 0.6 against levels of 0.01 .. 0.09 (asserted on the oracle's rows)
LOW, HIGH = 120.0, 900.0
PIECES = [(1,), (3, 1, 2), (4,)]
# the bank of Tiny models: train sizes -> gain windows 10 / 15 / 20 / 2 / 32; model 2 has no level
TRAIN = [30, 47, 61, 6, 96]
M_LEVELS = [0.05, 0.012, float("nan"), 0.09, 0.03]
M_NAN = 2
HIDDEN = 6
DET_MIN, DET_MAX = 0.5, 4.0          # the detector comparisons: reached by the loudest utterances and by the dithered silence
DET_KW = dict(gain_normalizer=True, min_gain=DET_MIN, max_gain=DET_MAX, band_pass=True, low_cutoff=80.0, high_cutoff=500.0)


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


def filters(ra, gain=True, band=True, gain_ref=None, min_gain=MIN_GAIN, max_gain=MAX_GAIN, low=LOW, high=HIGH):
    f = ra.FiltersConfig()
    f.gain_normalizer.enabled, f.gain_normalizer.min_gain, f.gain_normalizer.max_gain = gain, min_gain, max_gain
    f.gain_normalizer.gain_ref = gain_ref
    f.band_pass.enabled, f.band_pass.low_cutoff, f.band_pass.high_cutoff = band, low, high
    return f


# ------------------------------------------------------------------------------------------------ the two banks, as the oracle sees them

def ref_dicts():
    return [rpw_py.load_rpw(os.path.join(G, n)) for n in GOLDEN_RPW] + synth_dicts()


def tiny_model(i, L, level, seed=77):
    """a random Tiny model as tests/rpw_py.py and oracle.rp_oracle.Detector.add_model take it"""
    rng = np.random.default_rng(seed + i)
    dims = [L * 16, HIDDEN, 2]
    w = {}
    for l in range(2):
        w["ln%d.weight" % (l + 1)] = (rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l])).astype(np.float32)
        w["ln%d.bias" % (l + 1)] = (rng.standard_normal(dims[l + 1]) * 0.1).astype(np.float32)
    return {"labels": ["none", "a"], "train_size": L, "mfcc_size": 16, "m_type": "tiny", "weights": w, "rms_level": level}


def model_dicts():
    return [tiny_model(i, L, lv) for i, (L, lv) in enumerate(zip(TRAIN, M_LEVELS))]


def model_rpw(m):
    return rpw_py.dump_rpw_model(m["labels"], m["train_size"], m["mfcc_size"], m["m_type"], m["weights"], rms_level=m["rms_level"])


class Side:
    """one bank as the oracle needs it: window length and level of every entry, and the rows of the tests"""

    def __init__(self, kind, lens, levels, nan_w, loud_short, long_quiet, short, zero_window=None):
        self.kind, self.lens, self.levels, self.W = kind, list(lens), [np.float32(v) for v in levels], len(lens)
        self.nan_w, self.loud_short, self.long_quiet, self.short, self.zero_window = nan_w, loud_short, long_quiet, short, zero_window
        assert np.isnan(self.levels[nan_w])
        assert self.levels[loud_short] > self.levels[long_quiet] and self.lens[long_quiet] > self.lens[loud_short]

    def fold(self, row):
        """on_wakeword_change over the live slots of a row -> (target, Lmax), None for a detector without wakewords"""
        live = [int(w) for w in row if 0 <= w < self.W]
        if not live:
            return None
        lv = [self.levels[w] for w in live if not np.isnan(self.levels[w])]
        return (float(max(lv)) if lv else float("nan")), max(self.lens[w] for w in live)

    def rows(self, n, n_streams=S, seed=3):
        """[n_streams][n] indices: the named rows at the start of the batch, again in the partial last workgroup, random rows between"""
        pad = lambda r: (list(r) + [-1] * n)[:n]
        a, b = self.loud_short, self.long_quiet
        named = [pad([]),                                   # all -1
                 pad([a]),                                  # one live slot, the first
                 [-1] * (n - 1) + [b],                      # ... the last
                 pad([a, -1, b]),                           # -1 in the middle
                 [b] * n,                                   # duplicates
                 [self.nan_w] * n,                          # every level NaN: gain 1 throughout
                 pad([self.nan_w, b]) if n > 1 else [self.nan_w],   # the NaN entry beside a real one
                 pad([a, b]) if n > 1 else [a],             # the largest level and the longest window in different slots
                 pad([b, a]) if n > 1 else [b]]
        if self.zero_window is not None:
            named.append(pad([self.zero_window]))           # Lmax / 3 == 0 -> a window of 1
        rng = np.random.default_rng(seed + n)
        out = np.where(rng.random((n_streams, n)) < 0.3, -1, rng.integers(0, self.W, (n_streams, n))).astype(np.int32)
        for i, r in enumerate(named):
            out[i] = r
            if n_streams - len(named) + i >= len(named):
                out[n_streams - len(named) + i] = r
        return out


@pytest.fixture(scope="module")
def dicts():
    return ref_dicts()


@pytest.fixture(scope="module")
def ww_side(dicts):
    lens = [max(len(t) for t in d["samples_features"].values()) for d in dicts]
    assert [max(L // 3, 1) for L in lens] == WINDOWS
    # alexa: the largest level (0.0575) at 126 frames; oye_casa_real: the longest window (168 frames) at the smallest level; wakeword 7: 2 frames
    return Side("sets", lens, [d["rms_level"] for d in dicts], NAN_W, 0, 2, 3, zero_window=7)   # short: wakeword 3, 22 frames at 0.05


@pytest.fixture(scope="module")
def m_side():
    assert [L // 3 for L in TRAIN] == [10, 15, 20, 2, 32]
    return Side("models", TRAIN, M_LEVELS, M_NAN, 3, 4, 3)   # model 3: 6 frames at 0.09; model 4: 96 frames at 0.03


@pytest.fixture(scope="module")
def bank(ra, ctx):
    return make_bank(ra, ctx)


@pytest.fixture(scope="module")
def mbank(ra, ctx):
    b = ra.ModelBank(ctx, rpw=[model_rpw(m) for m in model_dicts()])
    assert b.train_sizes == TRAIN
    return b


@pytest.fixture(scope="module")
def audio():
    return varying_noise(S, NC, np.random.default_rng(11), silent=20)


_ORACLE = {}


def oracle_rows(tag, dec, side, rows, band, gain_ref=None, first=0):
    """orc.frontend_stream per stream with target(s) and Lmax(s) // 3 -> (out, rms, gains) as [n][..] arrays.  tag names the audio (rows of
    it from `first`), so that streams of equal (level, window) in different tests share one oracle run"""
    out, rms, gains = [], [], []
    for s in range(dec.shape[0]):
        f = side.fold(rows[s])
        key = (tag, first + s, dec.shape[1], band, gain_ref) + ((None,) if f is None else (bits1(f[0]), f[1] // 3))
        if key not in _ORACLE:
            if f is None:   # a detector without wakewords: gain 1, the band-pass runs as on a live bank batch
                _ORACLE[key] = orc.frontend_stream(dec[s], band_pass=band, low_cutoff=LOW, high_cutoff=HIGH)
            else:
                _ORACLE[key] = orc.frontend_stream(dec[s], gain_normalizer=True, gain_ref=gain_ref, min_gain=MIN_GAIN, max_gain=MAX_GAIN,
                                                   rms_level_ref=f[0], window_size=f[1] // 3, band_pass=band, low_cutoff=LOW, high_cutoff=HIGH)
        o, r, g = _ORACLE[key]
        out.append(o); rms.append(r); gains.append(g)
    return np.stack(out), np.stack(rms), np.stack(gains)


def honest(side, rows, want_gains, n_chunks=NC, extremes=True):
    """the conditions that keep a comparison from passing on nothing, on the oracle's rows"""
    share = float(np.mean(want_gains != 1.0))
    assert share >= 1.0 / 3.0, share
    if extremes:
        assert np.any(want_gains == np.float32(MIN_GAIN)) and np.any(want_gains == np.float32(MAX_GAIN))
    folds = [side.fold(r) for r in rows]
    assert any(f is not None and not np.isnan(f[0]) and max(f[1] // 3, 1) < n_chunks for f in folds), "no window wraps"


def frontend(ctx, side, bank, mbank):
    return (lambda x, f, idx: ctx.frontend_bank_sets(x, f, bank, idx)) if side.kind == "sets" else (lambda x, f, idx: ctx.frontend_model_bank(x, f, mbank, idx))


def same(got, want):
    for name, a, b in zip(("rms", "gains", "pcm_out"), (got[1], got[2], got[0]), (want[1], want[2], want[0])):
        bad = np.argwhere(bits(a) != bits(b))
        assert len(bad) == 0, (name, len(bad), bad[:6].tolist())


# ------------------------------------------------------------------------------------------------ 1. whole recordings against the oracle

CASES = [(k, n, np.float32, True) for k in ("sets", "models") for n in (1, 3, 8)] + \
        [(k, 3, d, b) for k in ("sets", "models") for d, b in ((np.float32, False), (np.int16, True), (np.int16, False))]


@pytest.mark.parametrize("kind,n,dtype,band", CASES)
def test_whole_recordings_against_the_oracle(ra, ctx, bank, mbank, ww_side, m_side, audio, kind, n, dtype, band):
    """130 streams x 90 chunks, set_size 1 / 3 / 8, f32 and i16 input, band-pass on and off: pcm_out, rms and gains equal, as uint32,
    orc.frontend_stream with the stream's target(s) and Lmax(s) // 3.  The first and the last rows of the batch are the named ones."""
    side = ww_side if kind == "sets" else m_side
    rows = side.rows(n)
    raw, dec = as_format(audio, dtype)
    want = oracle_rows(np.dtype(dtype).name, dec, side, rows, band)
    honest(side, rows, want[2])
    gone = [s for s in range(S) if side.fold(rows[s]) is None or np.isnan(side.fold(rows[s])[0])]
    assert len(gone) >= 2 and np.all(want[2][gone] == 1.0)
    if n > 1:   # the NaN entry beside a real one is ignored; the level and the window come from different slots
        assert side.fold(rows[6]) == (float(side.levels[side.long_quiet]), side.lens[side.long_quiet])
        assert side.fold(rows[7]) == (float(side.levels[side.loud_short]), side.lens[side.long_quiet]) == side.fold(rows[8])
    same(frontend(ctx, side, bank, mbank)(raw, filters(ra, True, band), rows), want)


@pytest.mark.parametrize("kind", ["sets", "models"])
def test_whole_recordings_with_a_fixed_gain_ref(ra, ctx, bank, mbank, ww_side, m_side, audio, kind):
    """has_gain_ref: one level for every stream with a live slot (also where every level is NaN), the window still Lmax(s) // 3"""
    side = ww_side if kind == "sets" else m_side
    rows = side.rows(3)
    want = oracle_rows("float32", audio, side, rows, True, gain_ref=0.04)
    honest(side, rows, want[2])
    assert np.all(want[2][0] == 1.0) and np.any(want[2][5] != 1.0)   # no live slot: gain 1; every level NaN: the fixed level serves
    same(frontend(ctx, side, bank, mbank)(audio, filters(ra, True, True, gain_ref=0.04), rows), want)


@pytest.mark.parametrize("kind", ["sets", "models"])
@pytest.mark.parametrize("n_streams", [1, 63, 64, 65])
def test_stream_counts(ra, ctx, bank, mbank, ww_side, m_side, audio, kind, n_streams):
    """S around one workgroup of the preparation kernel, with a tail shorter than a chunk (never framed: copied)"""
    side = ww_side if kind == "sets" else m_side
    n = 480 * 40 + 77
    first = 1   # (row 0 has no live slot: S = 1 would compare nothing)
    x = np.ascontiguousarray(audio[first:first + n_streams, :n])
    rows = side.rows(3)[first:first + n_streams]
    want_out = oracle_rows("float32", x, side, rows, True, first=first)[0]
    _, want_rms, want_gains = oracle_rows("float32", np.ascontiguousarray(x[:, :480 * 40]), side, rows, True, first=first)
    assert np.mean(want_gains != 1.0) >= 1.0 / 3.0
    out, rms, gains = frontend(ctx, side, bank, mbank)(x, filters(ra), rows)
    assert rms.shape == (n_streams, 40)
    same((out, rms, gains), (want_out, want_rms, want_gains))
    assert np.array_equal(out[:, 480 * 40:], x[:, 480 * 40:])


def test_device_pointer_context(ra, ww_side, m_side, audio):
    """A context without RP_CTX_HOST_POINTERS: audio, indices and outputs on the device, input and output rows with pitches of their own; an
    index outside the bank counts as -1"""
    import torch
    dctx = ra.BatchContext(device=0, host_pointers=False)
    dbank = make_bank(ra, dctx)
    dmbank = ra.ModelBank(dctx, rpw=[model_rpw(m) for m in model_dicts()])
    N, PIN, POUT = NC * 480, NC * 480 + 16, NC * 480 + 8
    raw, dec = as_format(audio, np.int16)
    d_pcm = torch.zeros((S, PIN), dtype=torch.int16, device="cuda")
    d_pcm[:, :N] = torch.from_numpy(raw).cuda()
    f = filters(ra)
    for side, bk, call in ((ww_side, dbank, dctx.frontend_bank_sets_dev), (m_side, dmbank, dctx.frontend_model_bank_dev)):
        rows = side.rows(3)
        want = oracle_rows("int16", dec, side, rows, True)
        honest(side, rows, want[2])
        bad = rows.copy()
        assert rows[0, 0] == -1 and rows[3, 1] == -1
        bad[0, 0], bad[3, 1] = side.W, -9
        d_idx = torch.from_numpy(bad).cuda()
        d_out = torch.full((S, POUT), 7.0, dtype=torch.float32, device="cuda")
        d_rms = torch.zeros((S, NC), dtype=torch.float32, device="cuda")
        d_gain = torch.zeros((S, NC), dtype=torch.float32, device="cuda")
        call(d_pcm.data_ptr(), 1, S, N, PIN, f, bk, d_idx.data_ptr(), 3, d_out.data_ptr(), POUT, d_rms.data_ptr(), d_gain.data_ptr())
        dctx.synchronize()
        out = d_out.cpu().numpy()
        same((out[:, :N], d_rms.cpu().numpy(), d_gain.cpu().numpy()), want)
        assert np.all(out[:, N:] == 7.0)


# ------------------------------------------------------------------------------------------------ 2. live = whole

def live_config(ra):
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold, cfg.min_scores = 0.0, 0.3, 2
    return cfg


def live_batch(ra, ctx, kind, bank, mbank, rows, f, max_chunks, cfg=None, n_streams=None):
    """kind: sets (rp_stream_batch_new_bank_sets), model (rp_stream_batch_new_model_bank, rows [S][1]) or model_sets"""
    n_streams = len(rows) if n_streams is None else n_streams
    kw = dict(max_chunks_per_call=max_chunks, per_stream_filters=f)
    cfg = cfg or live_config(ra)
    if kind == "sets":
        return ra.StreamBatch(ctx, None, cfg, n_streams, bank=bank, stream_wakewords=rows, **kw)
    if kind == "model":
        return ra.StreamBatch(ctx, None, cfg, n_streams, model_bank=mbank, stream_model=np.ascontiguousarray(rows[:, 0]), **kw)
    return ra.StreamBatch(ctx, None, cfg, n_streams, model_bank=mbank, stream_models=rows, **kw)


@pytest.mark.parametrize("kind", ["sets", "model", "model_sets"])
@pytest.mark.parametrize("pieces", PIECES)
def test_live_equals_whole(ra, ctx, bank, mbank, ww_side, m_side, audio, kind, pieces):
    """The same banks, rows and audio fed in pieces to the three kinds of batch: every call's rp_stream_batch_levels are the rows of the
    whole-recording call -- the oracle's -- bit for bit"""
    side = ww_side if kind == "sets" else m_side
    rows = side.rows(1 if kind == "model" else 3)
    raw, dec = as_format(audio, np.int16)
    want = oracle_rows("int16", dec, side, rows, True)
    honest(side, rows, want[2])
    whole = frontend(ctx, side, bank, mbank)(raw, filters(ra), rows)
    same(whole, want)
    sb = live_batch(ra, ctx, kind, bank, mbank, rows, filters(ra), max(pieces))
    _, _, rms, gains = feed(sb, raw, pieces)
    assert np.array_equal(bits(rms), bits(whole[1]))
    assert np.array_equal(bits(gains), bits(whole[2])), np.argwhere(gains != whole[2])[:8].tolist()


# ------------------------------------------------------------------------------------------------ 3. the oracle's chunk-wise detector

def feed_multi(sb, pcm, n_chunks, max_det=8):
    """pcm [S][C * 480] in calls of n_chunks through process_multi -> (per stream [(frame, window, counter, score, avg_score, bank index,
    label)], rms [S][C], gains [S][C])"""
    n_streams, total = pcm.shape[0], pcm.shape[1] // 480
    got, rms, gains = [[] for _ in range(n_streams)], [], []
    for c in range(0, total, n_chunks):
        n = min(n_chunks, total - c)
        det, dww, dlab, n_det = sb.process_multi(np.ascontiguousarray(pcm[:, c * 480:(c + n) * 480]), max_det=max_det)
        for s in range(n_streams):
            assert n_det[s] <= max_det
            for i in range(n_det[s]):
                d = det[s][i]
                got[s].append((int(d["frame"]), int(d["window"]), int(d["counter"]), float(d["score"]), float(d["avg_score"]), int(dww[s][i]), int(dlab[s][i])))
        lr, lg = sb.levels()
        rms.append(lr); gains.append(lg)
    return got, np.concatenate(rms, axis=1), np.concatenate(gains, axis=1)


def detector_run(d, pcm_i16):
    return [(c, r) for c in range(len(pcm_i16) // 480) for r in [d.process_i16(pcm_i16[c * 480:(c + 1) * 480])] if r is not None]


def test_sets_against_the_chunkwise_oracle_detector(ra, ctx, bank, dicts, ww_side):
    """Streams of the golden utterances at different loudness, each holding a set of wakewords, both filters on, through a live sets batch
    and one by one through orc.Detector with add_ref per live slot in slot order: the same detections (chunk, counter and winner exact,
    scores to 1e-5), the detection's gain is the live gain of its best window's chunk, and every chunk's level and gain equal the oracle's
    front-end with target(s) and Lmax(s) // 3."""
    rng = np.random.default_rng(31)
    oye, alexa = ("oye_casa_g_1.wav", "oye_casa_g_2.wav"), ("alexa.wav", "alexa2.wav")
    plan = [(oye, [1, 3, -1], 0.2, 5.0), (oye, [3, 1, 0], 0.5, 2.0), (alexa, [0, 4, 1], 0.5, 2.0), (alexa, [-1, 0, -1], 1.0, 0.3), (oye, [0, 1, 2], 0.5, 2.0)]
    streams = [utterances(f, g1, g2, rng) for f, _, g1, g2 in plan]
    n = (min(len(s) for s in streams) // 480) * 480
    pcm = np.stack([s[:n] for s in streams])
    rows = np.array([r for _, r, _, _ in plan], np.int32)
    # the oracle's side first
    want, levels = [], []
    for s, row in enumerate(rows):
        d = orc.Detector(avg_threshold=0.0, threshold=0.5, **DET_KW)
        for w in row:
            if w >= 0:
                d.add_ref(dicts[w])
        want.append(detector_run(d, pcm[s]))
        target, lmax = ww_side.fold(row)
        levels.append(orc.frontend_stream(simstream.i16_to_f32(pcm[s]), rms_level_ref=target, window_size=lmax // 3, **DET_KW))
    want_gains = np.stack([g for _, _, g in levels])
    assert sum(1 for w in want if w) >= 2, [len(w) for w in want]
    assert np.mean(want_gains != 1.0) >= 1.0 / 3.0 and np.any(want_gains == np.float32(DET_MIN)) and np.any(want_gains == np.float32(DET_MAX))
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold = 0.0, 0.5
    f = filters(ra, True, True, min_gain=DET_MIN, max_gain=DET_MAX, low=80.0, high=500.0)
    sb = live_batch(ra, ctx, "sets", bank, None, rows, f, 3, cfg=cfg)
    got, rms, gains = feed_multi(sb, pcm, 3)
    winners = set()
    for s, row in enumerate(rows):
        lmax = ww_side.fold(row)[1]
        assert np.array_equal(bits(rms[s]), bits(levels[s][1])) and np.array_equal(bits(gains[s]), bits(levels[s][2])), s
        assert len(got[s]) == len(want[s]), (s, got[s], want[s])
        for rec, (chunk, r) in zip(got[s], want[s]):
            best_chunk = (rec[1] + lmax - 1) // 3 + 1
            print(s, chunk, r["name"], r["counter"], float(r["score"]), rec[3], float(r["gain"]), float(gains[s][best_chunk]))
            assert rec[0] // 3 + 1 == chunk and rec[2] == r["counter"] and dicts[rec[5]]["name"] == r["name"], (s, rec, chunk, r)
            assert abs(rec[3] - float(r["score"])) <= 1e-5 * float(r["score"])
            assert gains[s][best_chunk] == r["gain"]
            winners.add(rec[5])
    assert len(winners) >= 2, winners


def golden_model(level):
    m = rpw_py.load_rpw(os.path.join(G, "ok_casa-tiny.rpw"))
    m["rms_level"] = level
    return m


def ok_casa_stream(gain, rng):
    """3 s of silence around tests/golden/ok_casa.wav at `gain`, +-12 of dither"""
    z = np.zeros(16000 * 3, np.int16)
    s = np.concatenate([z, simstream._read_raw(os.path.join(G, "ok_casa.wav"), gain), z])
    return (s.astype(np.int32) + rng.integers(-12, 13, len(s))).clip(-32768, 32767).astype(np.int16)


@pytest.mark.parametrize("kind", ["model", "model_sets"])
def test_models_against_the_chunkwise_oracle_detector(ra, ctx, m_side, kind):
    """The same for a model bank and for model sets: the five Tiny models and the golden ok_casa model (195 frames, given a level) on the
    golden recording at four loudnesses, against orc.Detector with add_model per live slot: detections exact (chunk, counter, winner and
    label), scores within 1e-5 (the bar tests/test_gpu_stream_model_bank.py holds against the oracle), gains bit for bit."""
    GOLD = 5
    ms = model_dicts() + [golden_model(0.02)]
    side = Side("models", TRAIN + [195], M_LEVELS + [0.02], M_NAN, 3, 4, 3)
    mb = ra.ModelBank(ctx, rpw=[model_rpw(m) for m in ms])
    assert bits1(mb.rms_levels[GOLD]) == bits1(0.02)
    rng = np.random.default_rng(5)
    rows = np.array([[GOLD, -1, -1], [GOLD, 0, -1], [1, GOLD, 3], [0, -1, -1], [-1, M_NAN, GOLD]] if kind == "model_sets" else [[GOLD], [GOLD], [GOLD], [0], [-1]], np.int32)
    streams = [ok_casa_stream(g, rng) for g in (1.0, 0.3, 2.0, 1.0, 0.5)]
    n = (min(len(s) for s in streams) // 480) * 480
    pcm = np.stack([s[:n] for s in streams])
    want, levels = [], []
    for s, row in enumerate(rows):
        d = orc.Detector(avg_threshold=0.0, threshold=0.5, min_scores=1, **DET_KW)
        for w in row:
            if w >= 0:
                d.add_model(ms[w])
        want.append(detector_run(d, pcm[s]))
        f = side.fold(row)
        levels.append(orc.frontend_stream(simstream.i16_to_f32(pcm[s]), band_pass=True, low_cutoff=80.0, high_cutoff=500.0) if f is None else
                      orc.frontend_stream(simstream.i16_to_f32(pcm[s]), rms_level_ref=f[0], window_size=f[1] // 3, **DET_KW))
    want_gains = np.stack([g for _, _, g in levels])
    assert sum(1 for w in want if w) >= 2, [len(w) for w in want]
    assert np.mean(want_gains != 1.0) >= 1.0 / 3.0 and np.any(want_gains == np.float32(DET_MIN)) and np.any(want_gains == np.float32(DET_MAX))
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold, cfg.min_scores = 0.0, 0.5, 1
    f = filters(ra, True, True, min_gain=DET_MIN, max_gain=DET_MAX, low=80.0, high=500.0)
    sb = live_batch(ra, ctx, kind, None, mb, rows, f, 8, cfg=cfg)
    got, rms, gains = feed_multi(sb, pcm, 8, max_det=12)
    n_det, worst = 0, 0.0
    for s, row in enumerate(rows):
        assert np.array_equal(bits(rms[s]), bits(levels[s][1])) and np.array_equal(bits(gains[s]), bits(levels[s][2])), s
        assert len(got[s]) == len(want[s]), (s, got[s], want[s])
        for rec, (chunk, r) in zip(got[s], want[s]):
            lmax = side.fold(row)[1]
            best_chunk = (rec[1] + lmax - 1) // 3 + 1
            print(s, chunk, r["name"], r["counter"], float(r["score"]), rec[3], float(r["gain"]), float(gains[s][best_chunk]))
            assert rec[0] // 3 + 1 == chunk and rec[2] == r["counter"] and ms[rec[5]]["labels"][rec[6]] == r["name"], (s, rec, chunk, r)
            worst = max(worst, abs(rec[3] - float(r["score"])), abs(rec[4] - float(r["avg_score"])))
            assert gains[s][best_chunk] == r["gain"]
            n_det += 1
    print("%d detections, worst score difference against the oracle %.3g" % (n_det, worst))
    assert worst <= 1e-5


# ------------------------------------------------------------------------------------------------ 4. retargeting, banks that change

def retarget_plan(side):
    """rows A (the longest window, level of another slot) and B (a short window, another level), and the chunk levels' window of A"""
    a, b = side.long_quiet, side.short
    A = [a, side.nan_w, -1]
    B = [-1, b, b]
    return A, B, side.fold(A), side.fold(B)


@pytest.mark.parametrize("kind", ["sets", "model", "model_sets"])
def test_retarget_mid_stream(ra, ctx, bank, mbank, ww_side, m_side, kind):
    """Gain normaliser alone, on noise.  Stream 0 goes from a long-window set A to a short one B at chunk C0 and back at C1: remove-all plus
    add-in-order set a new level and window size and leave the window of chunk levels as it is; filter() drops one level per push, so the
    window keeps the length it had -- the gains are those of A's window with B's level, NOT those of B's window.  Stream 1 goes to all -1
    for chunks 40 .. 49 and back: gain 1 meanwhile, its window goes on from what it held.  Stream 2 is never touched."""
    side = ww_side if kind == "sets" else m_side
    n = 1 if kind == "model" else 3
    A, B, (lvA, lenA), (lvB, lenB) = retarget_plan(side)
    if n == 1:
        A, B = [side.long_quiet], [side.short]
        (lvA, lenA), (lvB, lenB) = side.fold(A), side.fold(B)
    wa, wb = lenA // 3, lenB // 3
    C0, C1, GAP, NCH = wa + 6, wa + 24, range(40, 50), wa + 40
    pcm = varying_noise(3, NCH, np.random.default_rng(21), silent=None)
    assert all(np.any(pcm[s][c * 480:(c + 1) * 480] != 0) for s in range(3) for c in range(NCH))   # every level enters the window
    kw = dict(gain_normalizer=True, min_gain=MIN_GAIN, max_gain=MAX_GAIN)
    keep_a = orc.frontend_stream(pcm[0], rms_level_ref=lvA, window_size=wa, **kw)[2]
    keep_b = orc.frontend_stream(pcm[0], rms_level_ref=lvB, window_size=wa, **kw)[2]
    shrunk = orc.frontend_stream(pcm[0], rms_level_ref=lvB, window_size=wb, **kw)[2]
    want0 = np.concatenate([keep_a[:C0], keep_b[C0:C1], keep_a[C1:]])
    assert int(np.sum(want0[C0:C1] != shrunk[C0:C1])) >= 5, "this audio does not tell an unshrunk window from B's window"
    no_gap = np.concatenate([pcm[1][:GAP[0] * 480], pcm[1][(GAP[-1] + 1) * 480:]])
    g = orc.frontend_stream(no_gap, rms_level_ref=lvB, window_size=wb, **kw)[2]
    want1 = np.concatenate([g[:GAP[0]], np.ones(len(GAP), np.float32), g[GAP[0]:]])
    through = orc.frontend_stream(pcm[1], rms_level_ref=lvB, window_size=wb, **kw)[2]
    assert int(np.sum(want1[GAP[-1] + 1:] != through[GAP[-1] + 1:])) >= 1, "the gap leaves no trace in this audio"
    want2 = orc.frontend_stream(pcm[2], rms_level_ref=lvA, window_size=wa, **kw)[2]
    want = np.stack([want0, want1, want2])
    assert np.mean(want != 1.0) >= 1.0 / 3.0 and wa < C0
    rows = np.array([A, B, A], np.int32)
    sb = live_batch(ra, ctx, kind, bank, mbank, rows, filters(ra, True, False), 2)
    setter = {"sets": sb.set_wakeword_sets, "model": sb.set_models, "model_sets": sb.set_model_sets}[kind]
    shape = (lambda r: np.array(r, np.int32)) if kind == "model" else (lambda r: np.array([r], np.int32))

    def act(c):
        if c == C0:
            setter(0, shape(B))
        if c == C1:
            setter(0, shape(A))
        if c == GAP[0]:
            setter(1, shape([-1] * n))
        if c == GAP[-1] + 1:
            setter(1, shape(B))
    _, _, rms, gains = feed(sb, pcm, (1,), before_chunk=act)
    for s in range(3):
        assert np.array_equal(bits(gains[s]), bits(want[s])), (s, np.argwhere(gains[s] != want[s]).ravel().tolist())
    assert np.all(gains[1][GAP[0]:GAP[-1] + 1] == 1.0)


def test_retarget_against_the_oracle_detector(ra, ctx, bank, dicts, ww_side):
    """The same slot changes through orc.Detector: remove() of every wakeword, then add_ref in slot order.  Every scored window reports
    (threshold 0, one score is enough, eager), and each detection carries the gain of its best window's chunk: those are the live gains."""
    A, B, (lvA, lenA), (lvB, lenB) = retarget_plan(ww_side)
    C0, C1, NCH = 62, 80, 96
    pcm = varying_noise(1, NCH, np.random.default_rng(21), silent=None)
    kw = dict(gain_normalizer=True, min_gain=MIN_GAIN, max_gain=MAX_GAIN)
    okw = dict(avg_threshold=0.0, threshold=0.0, min_scores=1, eager=True, **kw)

    def swap(row):
        def go(d):
            while d.remove(0):
                pass
            for w in row:
                if w >= 0:
                    d.add_ref(dicts[w])
        return go
    d = orc.Detector(**okw)
    swap(A)(d)
    want = []
    for c in range(NCH):
        if c == C0:
            swap(B)(d)
        if c == C1:
            swap(A)(d)
        r = d.process_f32(pcm[0][c * 480:(c + 1) * 480])
        if r is not None:
            want.append((c, r))
    assert sum(1 for c, _ in want if C0 <= c < C1) >= 2 and sum(1 for c, r in want if r["gain"] != 1.0) >= len(want) // 3, [(c, float(r["gain"])) for c, r in want]
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold, cfg.min_scores, cfg.eager = 0.0, 0.0, 1, True
    sb = live_batch(ra, ctx, "sets", bank, None, np.array([A], np.int32), filters(ra, True, False), 1, cfg=cfg)

    def act(c):
        if c == C0:
            sb.set_wakeword_sets(0, np.array([B], np.int32))
        if c == C1:
            sb.set_wakeword_sets(0, np.array([A], np.int32))
    got, _, rms, gains = feed(sb, pcm, (1,), before_chunk=act)
    assert len(got[0]) == len(want), (got[0], [(c, r["counter"]) for c, r in want])
    for rec, (chunk, r) in zip(got[0], want):
        lmax = lenB if C0 <= chunk < C1 else lenA
        best_chunk = (rec[1] + lmax - 1) // 3 + 1
        assert rec[0] // 3 + 1 == chunk and rec[2] == r["counter"], (rec, chunk, r)
        assert gains[0][best_chunk] == r["gain"], (chunk, best_chunk, float(gains[0][best_chunk]), float(r["gain"]))


def test_a_bank_changed_under_the_batch(ra, ctx, dicts, audio):
    """put replaces a wakeword a sets batch holds by one of another length and level, rp_model_bank_set_rms_levels changes a model's level:
    the next process call works with the new values.  A window that becomes longer grows from what it held: from chunk C on the gains are
    those of a detector with the new window that started w_old chunks before C."""
    C0, NCH = 30, 70
    pcm = np.ascontiguousarray(audio[40:42, :NCH * 480])
    assert all(np.any(pcm[s][c * 480:(c + 1) * 480] != 0) for s in range(2) for c in range(NCH))
    kw = dict(gain_normalizer=True, min_gain=MIN_GAIN, max_gain=MAX_GAIN)
    f = filters(ra, True, False)
    # a wakeword bank of its own: the batch holds wakewords 3 (22 frames, 0.05) and 5 (4 frames); wakeword 3 becomes 66 frames at 0.08, the largest level of both rows
    bk = make_bank(ra, ctx)
    rows = np.array([[5, 3, -1], [3, -1, -1]], np.int32)
    new = {"name": "longer", "samples_features": {"t%d" % t: m for t, m in enumerate(orc.synth_templates(991, 3, 66, 5))}}
    old = [orc.frontend_stream(pcm[s], rms_level_ref=0.05, window_size=7, **kw)[2] for s in range(2)]
    grown = [orc.frontend_stream(pcm[s][(C0 - 7) * 480:], rms_level_ref=0.08, window_size=22, **kw)[2][7:] for s in range(2)]
    same_len = [orc.frontend_stream(pcm[s], rms_level_ref=0.08, window_size=7, **kw)[2][C0:] for s in range(2)]
    want = np.stack([np.concatenate([old[s][:C0], grown[s]]) for s in range(2)])
    assert np.mean(want != 1.0) >= 1.0 / 3.0 and all(int(np.sum(grown[s] != same_len[s])) >= 3 and int(np.sum(grown[s] != old[s][C0:])) >= 3 for s in range(2))
    sb = live_batch(ra, ctx, "sets", bk, None, rows, f, 2)
    _, _, _, gains = feed(sb, pcm, (2, 1), before_chunk=lambda c: bk.put_rpw(3, [rpw_py.dump_rpw_ref(new["name"], new["samples_features"], rms_level=0.08)]) if c == C0 else None)
    assert bk.max_lens[3] == 66 and bits1(bk.rms_levels[3]) == bits1(0.08)
    assert np.array_equal(bits(gains), bits(want)), np.argwhere(gains != want)[:8].tolist()
    sb.close()
    # a model bank of its own: model 0 (window 10) goes from 0.05 to 0.015, model 2 gets its first level
    mb = ra.ModelBank(ctx, rpw=[model_rpw(m) for m in model_dicts()])
    for kind, rows in (("model", np.array([[0], [2]], np.int32)), ("model_sets", np.array([[-1, 0, -1], [2, 2, -1]], np.int32))):
        mb.set_rms_levels(M_LEVELS)
        lv2 = [0.015, 0.012, 0.07, 0.09, 0.03]
        a = orc.frontend_stream(pcm[0], rms_level_ref=0.05, window_size=10, **kw)[2]
        b = orc.frontend_stream(pcm[0], rms_level_ref=0.015, window_size=10, **kw)[2]
        c2 = orc.frontend_stream(pcm[1][C0 * 480:], rms_level_ref=0.07, window_size=20, **kw)[2]   # no level before: the window was empty
        want = np.stack([np.concatenate([a[:C0], b[C0:]]), np.concatenate([np.ones(C0, np.float32), c2])])
        assert int(np.sum(a[C0:] != b[C0:])) >= 5 and np.mean(want != 1.0) >= 1.0 / 3.0
        sb = live_batch(ra, ctx, kind, None, mb, rows, f, 2)
        _, _, _, gains = feed(sb, pcm, (2, 1), before_chunk=lambda c: mb.set_rms_levels(lv2) if c == C0 else None)
        assert np.array_equal(bits(gains), bits(want)), (kind, np.argwhere(gains != want)[:8].tolist())
        sb.close()


# ------------------------------------------------------------------------------------------------ 5. a set of one is the one-wakeword call

def test_sets_of_one_are_the_bank_calls(ra, ctx, bank, ww_side, audio):
    """rp_frontend_batch_bank_sets with set_size 1 gives the bits of rp_frontend_batch_bank; rp_stream_batch_set_filters_per_stream on a
    one-wakeword bank batch those of rp_stream_batch_set_filters_bank: levels, gains, aggregates and detections"""
    idx = ww_side.rows(1)[:70, 0].copy()
    pcm = np.ascontiguousarray(audio[:70, :480 * 60])
    f = filters(ra)
    a = ctx.frontend_bank(pcm, f, bank, idx)
    b = ctx.frontend_bank_sets(pcm, f, bank, idx[:, None])
    assert np.mean(a[2] != 1.0) >= 1.0 / 3.0
    same(b, a)
    cfg = live_config(ra)
    A = ra.StreamBatch(ctx, None, cfg, 70, max_chunks_per_call=3, bank=bank, stream_wakeword=idx, bank_filters=f)
    B = ra.StreamBatch(ctx, None, cfg, 70, max_chunks_per_call=3, bank=bank, stream_wakeword=idx, per_stream_filters=f)
    ga, gb = feed(A, pcm, (3, 1, 2), want_agg=True), feed(B, pcm, (3, 1, 2), want_agg=True)
    assert ga[0] == gb[0] and all(np.array_equal(bits(x), bits(y)) for x, y in zip(ga[1:], gb[1:]))
    assert np.array_equal(bits(ga[3]), bits(a[2]))
    # the band-pass alone through the new call is rp_stream_batch_set_filters
    bp = filters(ra, False, True)
    rows = ww_side.rows(3)[:10]
    A = ra.StreamBatch(ctx, None, cfg, 10, max_chunks_per_call=3, bank=bank, stream_wakewords=rows, filters=bp)
    B = ra.StreamBatch(ctx, None, cfg, 10, max_chunks_per_call=3, bank=bank, stream_wakewords=rows, per_stream_filters=bp)
    ga, gb = feed(A, pcm[:10], (3,)), feed(B, pcm[:10], (3,))
    assert ga[0] == gb[0] and np.array_equal(bits(ga[2]), bits(gb[2])) and np.all(gb[3] == 1.0)


# ------------------------------------------------------------------------------------------------ 6. the levels of a model bank

def test_model_bank_levels(ra, ctx, audio):
    """kept from .rpw by _new_from_rpw / _put_from_rpw, the file's level after _train, NaN from handles; set / get, a NULL bank, an index
    outside the bank; the levels survive a pool move, on the device too"""
    from test_gpu_train_batch import LR, _models
    L = ra.load_library()
    ms = model_dicts()
    b = ra.ModelBank(ctx, rpw=[model_rpw(m) for m in ms])
    want = np.array(M_LEVELS, np.float32)
    eq = lambda x, y: np.array_equal(bits(x), bits(np.asarray(y, np.float32)))
    assert eq(b.rms_levels, want)
    # handles: no level; a replaced model gets its new level
    handle = ra.Model(ctx, [ms[1]["weights"]["ln1.weight"], ms[1]["weights"]["ln2.weight"]], [ms[1]["weights"]["ln1.bias"], ms[1]["weights"]["ln2.bias"]])
    b.put(1, [handle], none_index=[0])
    assert np.isnan(b.rms_levels[1]) and eq(np.delete(b.rms_levels, 1), np.delete(want, 1))
    b.put_rpw(1, [model_rpw(tiny_model(1, 47, 0.33))])
    assert bits1(b.rms_levels[1]) == bits1(0.33)
    assert np.all(np.isnan(ra.ModelBank(ctx, models=[handle, handle]).rms_levels))
    # set / get and their edges
    b.set_rms_levels(M_LEVELS)
    assert eq(b.rms_levels, want)
    assert np.isnan(L.rp_model_bank_rms_level(b._h, 5)) and np.isnan(L.rp_model_bank_rms_level(b._h, -1)) and np.isnan(L.rp_model_bank_rms_level(None, 0))
    assert L.rp_model_bank_set_rms_levels(b._h, None) == -1 and b"null argument" in L.rp_last_error()
    assert L.rp_model_bank_set_rms_levels(None, None) == -1 and b"null handle" in L.rp_last_error()
    with pytest.raises(ValueError):
        b.set_rms_levels([0.05])
    empty = ra.ModelBank(ctx, models=[])
    assert empty.rms_levels.shape == (0,)
    empty.set_rms_levels([])
    # a pool move: models appended until the pools have been replaced; every level is where it was, on the device too
    pcm = np.ascontiguousarray(audio[50:55, :480 * 50])
    idx = np.arange(5, dtype=np.int32)
    f = filters(ra, True, False)
    before = ctx.frontend_model_bank(pcm, f, b, idx)
    assert np.mean(before[2] != 1.0) >= 1.0 / 3.0
    grown, k = b.pool_growths, 0
    while b.pool_growths < grown + 2 and k < 40:
        b.put_rpw(b.W, [model_rpw(tiny_model(10 + k, 96, 0.001 * (k + 1)))])
        k += 1
    assert b.pool_growths >= grown + 2 and eq(b.rms_levels[:5], want) and eq(b.rms_levels[5:], [0.001 * (i + 1) for i in range(k)])
    same(ctx.frontend_model_bank(pcm, f, b, idx), before)
    last = ctx.frontend_model_bank(pcm[:1], f, b, np.array([b.W - 1], np.int32))[2]
    assert np.array_equal(bits(last[0]), bits(orc.frontend_stream(pcm[0], gain_normalizer=True, min_gain=MIN_GAIN, max_gain=MAX_GAIN, rms_level_ref=0.001 * k, window_size=32)[2]))
    # trained into the bank: the level the trained file carries
    t = ra.ModelBank(ctx, models=[])
    got = t.train(0, _models()[0:2], m_type="tiny", learning_rate=LR, epochs=1, seeds=[7, 8])
    file_levels = [rpw_py._dec(g[0], 0)[0]["rms_level"] for g in got]
    assert all(lv > 0 for lv in file_levels), file_levels
    assert eq(t.rms_levels, file_levels)


# ------------------------------------------------------------------------------------------------ 7. refusals

def test_refusals_leave_the_batch_as_it_was(ra, ctx, bank, mbank, dicts, ww_side, m_side, audio):
    """after audio, with 40 ms input in either order, on a shared-wakeword batch, with a bank of another context, with a host index outside
    the bank: each is refused with a message, and the batch goes on like a twin that never saw the call"""
    pcm = np.ascontiguousarray(audio[20:25, :480 * 12])
    f = filters(ra)
    cfg = live_config(ra)
    rows = ww_side.rows(3)[3:8]
    mrows = m_side.rows(3)[3:8]

    def same_run(a, b, x):
        ra_, rb = feed(a, x, (2, 1)), feed(b, x, (2, 1))
        assert ra_[0] == rb[0] and np.array_equal(bits(ra_[2]), bits(rb[2])) and np.array_equal(bits(ra_[3]), bits(rb[3]))

    make = {"sets": lambda **kw: ra.StreamBatch(ctx, None, cfg, 5, max_chunks_per_call=2, bank=bank, stream_wakewords=rows, **kw),
            "model": lambda **kw: ra.StreamBatch(ctx, None, cfg, 5, max_chunks_per_call=2, model_bank=mbank, stream_model=np.ascontiguousarray(mrows[:, 1]), **kw),
            "model_sets": lambda **kw: ra.StreamBatch(ctx, None, cfg, 5, max_chunks_per_call=2, model_bank=mbank, stream_models=mrows, **kw)}
    for kind, new in make.items():
        # after the first audio
        a, twin = new(per_stream_filters=f), new(per_stream_filters=f)
        a.process(pcm[:, :480]); twin.process(pcm[:, :480])
        with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_filters_per_stream: the streams have already received audio"):
            a.set_filters_per_stream(filters(ra, True, False))
        same_run(a, twin, pcm[:, 480:])
        # filters, then 22.05 kHz input; 22.05 kHz input, then filters
        a, twin = new(per_stream_filters=f), new(per_stream_filters=f)
        with pytest.raises(ra.RustpotterError, match="40 ms"):
            a.set_input(22050)
        assert a.samples_per_chunk == 480
        same_run(a, twin, pcm)
        a = new(sample_rate=22050)
        with pytest.raises(ra.RustpotterError, match="40 ms"):
            a.set_filters_per_stream(f)
        assert a.samples_per_chunk == 882
        a.process(np.ascontiguousarray(audio[20:25, :882 * 2]))
        with pytest.raises(ra.RustpotterError):
            a.levels()
        # the old calls still refuse, with the texts they had
        a = new()
        with pytest.raises(ra.RustpotterError, match="gain normaliser is not available on a batch over a (wakeword|model) bank"):
            a.set_filters(f, 0.05)
        with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_filters_bank: the gain normaliser"):
            a.set_filters_bank(f)
        a.set_filters_per_stream(f)   # ... and left the batch as it was
        same_run(a, new(per_stream_filters=f), pcm)
    # a batch of shared wakewords
    d = dicts[3]
    tm = ra.Templates(ctx, list(d["samples_features"].values()))
    a = ra.StreamBatch(ctx, tm, cfg, 5, max_chunks_per_call=2, filters=f, rms_level_ref=0.05)
    twin = ra.StreamBatch(ctx, tm, cfg, 5, max_chunks_per_call=2, filters=f, rms_level_ref=0.05)
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_filters_per_stream: the batch holds shared wakewords.*rp_stream_batch_set_filters takes them"):
        a.set_filters_per_stream(f)
    ra_, rb = feed(a, pcm, (2, 1), want_agg=True), feed(twin, pcm, (2, 1), want_agg=True)
    assert ra_[0] == rb[0] and all(np.array_equal(bits(x), bits(y)) for x, y in zip(ra_[1:], rb[1:]))
    # a host index outside the bank: nothing is written, the message names stream and slot
    L = ra.load_library()
    fc = ra.RustpotterConfig()
    fc.filters = f
    cf = fc._filters_c()
    for fn, bk, W, what in ((L.rp_frontend_batch_bank_sets, bank, 9, "wakeword index"), (L.rp_frontend_batch_model_bank, mbank, 5, "model index")):
        out = np.full((5, pcm.shape[1]), 7.0, np.float32)
        rms = np.full((5, 12), 7.0, np.float32)
        gains = np.full((5, 12), 7.0, np.float32)
        bad = np.array([[0, 1, -1], [1, -1, 2], [0, -1, W], [2, 2, 2], [-1, -1, -1]], np.int32)
        r = fn(ctx._h, pcm.ctypes.data, 3, 5, pcm.shape[1], pcm.shape[1], C.byref(cf), bk._h, bad.ctypes.data, 3, out.ctypes.data, pcm.shape[1],
               rms.ctypes.data, gains.ctypes.data)
        assert r == -1 and ("stream 2, slot 2: %s %d is outside the bank (-1 .. %d)" % (what, W, W - 1)).encode() in L.rp_last_error(), L.rp_last_error()
        assert np.all(out == 7.0) and np.all(rms == 7.0) and np.all(gains == 7.0)
        r = fn(ctx._h, pcm.ctypes.data, 3, 5, pcm.shape[1], pcm.shape[1], C.byref(cf), bk._h, bad.ctypes.data, 9, out.ctypes.data, pcm.shape[1],
               rms.ctypes.data, gains.ctypes.data)
        assert r == -1 and b"set_size 9 is outside 1 .. 8" in L.rp_last_error()
    with pytest.raises(ra.RustpotterError, match="stream 1, slot 0: wakeword index 9"):
        ra.StreamBatch(ctx, None, cfg, 5, max_chunks_per_call=2, bank=bank, stream_wakewords=rows, per_stream_filters=f).set_wakeword_sets(1, np.array([[9, 0, 0]], np.int32))
    other = ra.BatchContext(device=0, host_pointers=True)
    with pytest.raises(ra.RustpotterError, match="the bank belongs to another context"):
        other.frontend_bank_sets(pcm, f, bank, rows)
    with pytest.raises(ra.RustpotterError, match="the bank belongs to another context"):
        other.frontend_model_bank(pcm, f, mbank, mrows)
