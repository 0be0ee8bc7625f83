"""Mixed sets on live streams (rp_stream_batch_new_mixed_sets / _set_mixed_sets; mixed_targets_kernel, dtw_mixed_stream_kernel,
window_means_mixed_stream_kernel, mlp_mixed_stream_kernel, nn_score_set_stream_kernel, scan_mixed_set_stream_kernel): a live-stream batch in
which stream s holds wakeword references of a wakeword bank AND models of a model bank on one detector.  The window that ends at a new frame
starts Lmax(s) - 1 frames before it for every slot of either kind, with Lmax(s) over both rows.
Yardsticks: rp_batch_detect_mixed_sets over the concatenation (frame, window, counter, index and label exact; reference scores within 1e-5,
model scores within 2e-6), oracle.rp_oracle.Detector fed chunk by chunk (tests/mixed_set_cases.py), and any other cut of the audio into
calls (slot scores under RP_CTX_FULL_SCORES and logits bit for bit).  Calls of 1, (3, 1, 2) and 10 chunks bring 3, 9 / 3 / 6 and 30 new
frames: both row-tile builds of the forward, DTW waves that span streams of different Lmax with a partial last wave.
Bank, rows and audio: tests/mixed_set_cases.py; base configuration as tests/test_gpu_mixed_sets.py (eager, min_scores 2)."""
import ctypes as C

import numpy as np
import pytest

import mixed_set_cases as X
import model_set_cases as M
from oracle import rp_oracle as orc
from test_gpu_mixed_sets import config, f32, make_banks, same_as_oracle

pytestmark = pytest.mark.gpu
MAX_CHUNKS = 10
CUTS = [(1,), (3, 1, 2), (10,)]


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


@pytest.fixture(scope="module")
def full(ra):
    """a context that scores every window (RP_CTX_FULL_SCORES): slot scores that do not depend on the gate"""
    return ra.BatchContext(device=0, host_pointers=True, full_scores=True)


@pytest.fixture(scope="module")
def banks(ra, ctx):
    return make_banks(ra, ctx)


@pytest.fixture(scope="module")
def full_banks(ra, full):
    return make_banks(ra, full)


@pytest.fixture(scope="module")
def pcm():
    return X.pcm()


def batch(ra, c, banks, cfg, ref_rows=X.REF_ROWS, model_rows=X.MODEL_ROWS, **kw):
    return ra.StreamBatch(c, None, cfg, len(ref_rows), max_chunks_per_call=MAX_CHUNKS, bank=banks[0], stream_wakewords=ref_rows, model_bank=banks[1],
                          stream_models=model_rows, **kw)


def feed(sb, pcm, pieces, want_rows=False, before_chunk=None, levels=None):
    """pcm [S][C * 480] through the batch in calls of pieces[0], pieces[1], ... chunks (cycled) -> per stream the list of (frame, window,
    counter, score bits, avg bits, index, label); with want_rows the slot scores (agg, avg) and the logits of every call side by side along
    the frame axis; levels: a list that gets (rms, gains) of every call"""
    n_streams, total = pcm.shape[0], pcm.shape[1] // 480
    out, agg, avg, logits = [[] for _ in range(n_streams)], [], [], []
    c = k = 0
    while c < total:
        n = min(pieces[k % len(pieces)], total - c)
        k += 1
        if before_chunk is not None:
            before_chunk(c)
        det, dww, dlab, n_det = sb.process_multi(np.ascontiguousarray(pcm[:, c * 480:(c + n) * 480]), max_det=MAX_CHUNKS + 1)
        for s in range(n_streams):
            for i in range(n_det[s]):
                d = det[s][i]
                assert d["stream"] == s
                out[s].append((int(d["frame"]), int(d["window"]), int(d["counter"]), M.bits(d["score"]), M.bits(d["avg_score"]), int(dww[s][i]),
                               int(dlab[s][i])))
            assert not det[s][n_det[s]:].tobytes().strip(b"\0") and (dlab[s][n_det[s]:] == -1).all()
        if want_rows:
            a, v = sb.slot_scores()
            agg.append(a); avg.append(v); logits.append(sb.logits())
        if levels is not None:
            levels.append(sb.levels())
        c += n
    assert sb.chunks_seen == total
    if want_rows:
        return out, (np.concatenate(agg, axis=-1), np.concatenate(avg, axis=-1), np.concatenate(logits, axis=-2))
    return out, None


def same_rows(a, b):
    """windows that lie inside the audio: column j is the window that ends at frame j - 3 and starts Lmax(s) - 1 frames before it"""
    for s, (rr, mr, _, _) in enumerate(X.ROWS):
        first = max(X.lmax_of(rr, mr) - 1, 0) + 3
        for name, x, y in (("agg", a[0][s, :, first:], b[0][s, :, first:]), ("avg", a[1][s, :, first:], b[1][s, :, first:]),
                           ("logits", a[2][s, :, first:], b[2][s, :, first:])):
            assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), (s, name, int(np.sum(x.view(np.uint32) != y.view(np.uint32))))


@pytest.fixture(scope="module")
def one_chunk(ra, full, full_banks, pcm):
    """the reference run: calls of one chunk on the context that scores every window"""
    full.dtw_kernels()
    det, rows = feed(batch(ra, full, full_banks, config(ra, X.Cfg())), pcm, (1,), want_rows=True)
    assert full.dtw_kernels() == ["dtw_mixed_stream_kernel"]   # RP_DTW_KERNEL_MIXED_SETS_STREAM and only that bit
    assert rows[0].shape == rows[1].shape == (X.S, 2, 3 * X.CHUNKS) and rows[2].shape == (X.S, 2, 3 * X.CHUNKS, M.LABEL_PITCH)
    print("calls of 1 chunk: %s detections" % [len(d) for d in det])
    return det, rows


# ---------------------------------------------------------------------------------------------- 1. cuts, the whole call, the oracle

@pytest.mark.parametrize("pieces", CUTS)
def test_cuts_against_the_whole_recording_and_the_oracle(ra, ctx, banks, full, full_banks, pcm, one_chunk, pieces):
    cfg = config(ra, X.Cfg())
    det, _ = feed(batch(ra, ctx, banks, cfg), pcm, pieces)           # detect-only: the gate may leave windows unscored
    if pieces != (1,):
        fdet, rows = feed(batch(ra, full, full_banks, cfg), pcm, pieces, want_rows=True)
        assert fdet == one_chunk[0]
        same_rows(rows, one_chunk[1])
    assert det == one_chunk[0]
    # rp_batch_detect_mixed_sets over the concatenation
    wdet, wdw, wdl, wn = ctx.batch_detect_mixed_sets(pcm, banks[0], X.REF_ROWS, banks[1], X.MODEL_ROWS, cfg, max_det=32)
    total = 0
    for s in range(X.S):
        want = [(int(d["frame"]), int(d["window"]), int(d["counter"]), float(d["score"]), float(d["avg_score"]), int(wdw[s][j]), int(wdl[s][j]))
                for j, d in enumerate(wdet[s][:wn[s]])]
        assert [d[:3] + d[5:] for d in det[s]] == [w[:3] + w[5:] for w in want], (s, det[s], want)
        for d, w in zip(det[s], want):
            sc, av = f32(d[3]), f32(d[4])
            print("stream %d frame %d: live %.7f / %.7f, whole %.7f / %.7f" % (s, d[0], sc, av, w[3], w[4]))
            if d[6] >= 0:
                assert abs(sc - w[3]) <= 2e-6 and abs(av - w[4]) <= 2e-6, (s, d, w)
            else:
                assert abs(sc - w[3]) <= 1e-5 * w[3] and abs(av - w[4]) <= 1e-5 * max(w[4], 1e-30), (s, d, w)
        total += len(want)
    assert total >= 15
    # the oracle fed chunk by chunk
    c = X.Cfg()
    for s, (rr, mr, _, _) in enumerate(X.ROWS):
        same_as_oracle(s, rr, mr, det[s], X.oracle_detect(rr, mr, pcm[s], c), 3 * X.CHUNKS - 3)


def test_slot_rows_are_the_families(ra, full, full_banks, one_chunk, pcm):
    """a row without models gives the slot scores of a wakeword-sets batch, a row without references the logits of a model-sets batch, bit for
    bit: the combined Lmax(s) is then the side's own"""
    cfg = config(ra, X.Cfg())
    sets = ra.StreamBatch(full, None, cfg, X.S, max_chunks_per_call=MAX_CHUNKS, bank=full_banks[0], stream_wakewords=X.REF_ROWS)
    msets = ra.StreamBatch(full, None, cfg, X.S, max_chunks_per_call=MAX_CHUNKS, model_bank=full_banks[1], stream_models=X.MODEL_ROWS)
    for c in range(0, 60, 10):
        part = np.ascontiguousarray(pcm[:, c * 480:(c + 10) * 480])
        sets.process_multi(part)
        msets.process_multi(part)
    agg, avg = sets.slot_scores()
    lg = msets.logits()
    cols = slice(50 * 3, 60 * 3)
    for s, (rr, mr, _, _) in enumerate(X.ROWS):
        if max(mr) < 0 and max(rr) >= 0:
            assert np.array_equal(agg[s].view(np.uint32), one_chunk[1][0][s][:, cols].view(np.uint32)), s
            assert np.array_equal(avg[s].view(np.uint32), one_chunk[1][1][s][:, cols].view(np.uint32)), s
        if max(rr) < 0 and max(mr) >= 0:
            assert np.array_equal(lg[s].view(np.uint32), one_chunk[1][2][s][:, cols].view(np.uint32)), s


# ---------------------------------------------------------------------------------------------- 2. re-targeting

def oracle_retarget(before, after, x, at, cfg, **kw):
    """the oracle with the rows `before`; in front of chunk `at` every wakeword is removed and the rows `after` are added in order"""
    k = X.oracle_kwargs(cfg)
    k.update(kw)
    d = orc.Detector(**k)
    who = []

    def add(rows):
        for w in rows[0]:
            if w >= 0:
                d.add_ref(X.refs()[w]); who.append(("ref", int(w)))
        for m in rows[1]:
            if m >= 0:
                d.add_model(X.model_dicts()[m]); who.append(("model", int(m)))
    add(before)
    n_before = len(who)
    out = []
    x = np.ascontiguousarray(x, np.float32)
    for i in range(0, len(x) - 479, 480):
        if i // 480 == at:
            for _ in range(n_before):
                assert d.remove(0)
            add(after)
        det = orc.Detection()
        if orc.lib().orc_detector_process(d._h, x[i:i + 480].ctypes.data_as(C.POINTER(C.c_float)), C.byref(det)):
            kind, idx = who[det.wakeword]
            out.append((i // 480, kind, idx, int(det.name) if kind == "model" else -1, np.float32(det.score), np.float32(det.avg_score), int(det.counter)))
    return out


def test_set_mixed_sets_between_calls(ra, ctx, banks, pcm):
    """At chunk 40 stream 3 is re-targeted, stream 5 emptied and stream 6 (empty until then) connected: from there each behaves as the
    oracle whose wakewords were all removed and the new ones added in order at that chunk.  A refused row -- a bad index on either side --
    changes nothing."""
    c = X.Cfg()
    cfg = config(ra, c)
    sb = batch(ra, ctx, banks, cfg)
    new = {3: ((0, -1), (1, -1)), 5: ((-1, -1), (-1, -1)), 6: ((1, 0), (0, -1))}

    def retarget(chunk):
        if chunk != 40:
            return
        bad_r, bad_m = np.array([[0, 3]], np.int32), np.array([[6, -1]], np.int32)
        with pytest.raises(ra.RustpotterError, match="stream 3, slot 1: wakeword index 3"):
            sb.set_mixed_sets(3, bad_r, np.array([new[3][1]], np.int32))
        with pytest.raises(ra.RustpotterError, match="stream 3, slot 0: model index 6"):
            sb.set_mixed_sets(3, np.array([new[3][0]], np.int32), bad_m)
        with pytest.raises(ra.RustpotterError, match="reach past the batch's %d streams" % X.S):
            sb.set_mixed_sets(X.S - 1, X.REF_ROWS[:2], X.MODEL_ROWS[:2])
        sb.set_mixed_sets(3, np.array([new[3][0]], np.int32), np.array([new[3][1]], np.int32))
        sb.set_mixed_sets(5, np.array([new[5][0], new[6][0]], np.int32), np.array([new[5][1], new[6][1]], np.int32))
    det, _ = feed(sb, pcm, (4,), before_chunk=retarget)
    nf = 3 * X.CHUNKS - 3
    fired = 0
    for s, (rr, mr, _, _) in enumerate(X.ROWS):
        if s in new:
            want = oracle_retarget((rr, mr), new[s], pcm[s], 40, c)
            assert len(det[s]) == len(want), (s, det[s], want)
            for g, w in zip(det[s], want):
                row = new[s] if g[0] >= 120 else (rr, mr)
                same_as_oracle(s, row[0], row[1], [g], [w], nf)
                fired += g[0] >= 120
        else:
            same_as_oracle(s, rr, mr, det[s], X.oracle_detect(rr, mr, pcm[s], c), nf)
    assert not [g for g in det[5] if g[0] >= 120] and fired >= 2


# ---------------------------------------------------------------------------------------------- 3. a bank that changes under the batch

def test_a_longer_model_put_under_the_batch(ra, ctx, pcm):
    """Stream 0 holds the 42-frame reference and model index 1 (47 frames): Lmax 47.  At chunk 42 a 96-frame model is put at index 1, within
    the model bank's reservation (96).  From the next call the stream's window, countdown and the reference slot's frames follow Lmax = 96,
    as the oracle whose model was replaced then (remove-all plus add, which resets); a model beyond the reservation is refused."""
    weights = M.bank_weights()
    bank = ra.WakewordBank(ctx, wakewords=X.bank_wakewords()[:1])
    mb = ra.ModelBank(ctx, models=[ra.Model(ctx, *weights[i]) for i in (0, 1)], none_index=[0, 0])
    mb.reserve(max_train_size=96, max_labels=3)
    c = X.Cfg()
    cfg = config(ra, c)
    rr, mr = np.array([[0, -1], [0, -1]], np.int32), np.array([[1, -1], [-1, 0]], np.int32)
    x = pcm[[7, 3]]
    sb = ra.StreamBatch(ctx, None, cfg, 2, max_chunks_per_call=MAX_CHUNKS, bank=bank, stream_wakewords=rr, model_bank=mb, stream_models=mr)

    def grow(chunk):
        if chunk == 42:
            mb.put(1, [ra.Model(ctx, *weights[2])], none_index=[M.NONE_INDEX[2]])     # index 1: L 47 -> 96
            with pytest.raises(ra.RustpotterError, match="195"):
                mb.put(0, [ra.Model(ctx, *weights[3])], none_index=[0])
            sb.set_mixed_sets(0, rr[:1], mr[:1])   # add_wakeword on the detector: a reset, as the reference does
    det, _ = feed(sb, x, (6,), before_chunk=grow)
    want = oracle_retarget(((0, -1), (1, -1)), ((0, -1), (2, -1)), x[0], 42, c)
    nf = 3 * X.CHUNKS - 3
    assert len(det[0]) == len(want), (det[0], want)
    after = 0
    for g, w in zip(det[0], want):
        new = g[0] >= 126
        same_as_oracle(0, (0, -1), (2, -1) if new else (1, -1), [(g[0], g[1], g[2], g[3], g[4], 2 if (new and g[6] >= 0) else g[5], g[6])], [w], nf)
        if new:
            assert 126 <= g[1] <= g[0] - 96 + 1, g     # windows of the new Lmax, none reaching before the reset
            after += 1
    assert after >= 1, (det[0], want)
    # the other stream never noticed
    same_as_oracle(1, (0, -1), (-1, 0), det[1], X.oracle_detect((0, -1), (-1, 0), x[1], c), nf)
    sb.close()


# ---------------------------------------------------------------------------------------------- 4. the gain normaliser

def test_gain_normaliser_per_stream(ra, ctx, pcm):
    """rp_stream_batch_set_filters_per_stream: levels and gains of every chunk equal oracle.frontend_stream with the largest non-NaN level
    over BOTH rows and max(Lmax(s) / 3, 1) levels, as uint32; the detections are the oracle detector's with the same filters.  Stream 3 is
    re-targeted at chunk 40 to rows of the same Lmax and another level: it keeps its window of chunk levels (its gains from there are those
    of a stream that worked towards the new level from the start)."""
    from test_gpu_bank_filters import bits
    bank, mbank = make_banks(ra, ctx)
    ref_levels = np.array([2e-4, float("nan"), 6e-4], np.float32)
    model_levels = np.array([5e-4, 1e-4, float("nan"), 3e-4, float("nan"), 9e-4], np.float32)
    bank.set_rms_levels(ref_levels)
    mbank.set_rms_levels(model_levels)
    f = ra.FiltersConfig()
    f.gain_normalizer.enabled, f.gain_normalizer.min_gain, f.gain_normalizer.max_gain = True, 0.05, 8.0
    c = X.Cfg()
    cfg = config(ra, c)
    sb = batch(ra, ctx, (bank, mbank), cfg, per_stream_filters=f)
    new3 = ((1, -1), (5, -1))     # Lmax 120 as before, the level 9e-4 of model 5 in the place of model 0's 5e-4

    def retarget(chunk):
        if chunk == 40:
            sb.set_mixed_sets(3, np.array([new3[0]], np.int32), np.array([new3[1]], np.int32))
    lv = []
    det, _ = feed(sb, pcm, (4,), before_chunk=retarget, levels=lv)
    rms, gains = np.concatenate([a for a, _ in lv], axis=1), np.concatenate([b for _, b in lv], axis=1)

    def target(rr, mr):
        v = [ref_levels[w] for w in rr if w >= 0] + [model_levels[m] for m in mr if m >= 0]
        v = [x for x in v if not np.isnan(x)]
        return max(v) if v else None
    kw = dict(gain_normalizer=True, min_gain=0.05, max_gain=8.0)   # wide enough that the levels of the quiet stretches do not all clip
    moved = 0
    for s, (rr, mr, _, _) in enumerate(X.ROWS):
        t, lmax = target(rr, mr), X.lmax_of(rr, mr)
        want = orc.frontend_stream(pcm[s]) if t is None else orc.frontend_stream(pcm[s], rms_level_ref=float(t), window_size=max(lmax // 3, 1), **kw)
        assert np.array_equal(bits(rms[s]), bits(want[1])), s
        if s == 3:
            assert X.lmax_of(*new3) == lmax and target(*new3) != t
            later = orc.frontend_stream(pcm[s], rms_level_ref=float(target(*new3)), window_size=max(lmax // 3, 1), **kw)
            assert np.array_equal(bits(gains[s][:40]), bits(want[2][:40])) and np.array_equal(bits(gains[s][40:]), bits(later[2][40:])), s
            assert not np.array_equal(bits(want[2][40:]), bits(later[2][40:]))
            continue
        assert np.array_equal(bits(gains[s]), bits(want[2])), s
        moved += int(np.sum(want[2] != 1.0))
        if t is None:
            assert (gains[s] == 1.0).all()
        got = X.oracle_detect(rr, mr, pcm[s], c, ref_levels=ref_levels, model_levels=model_levels, **kw)
        same_as_oracle(s, rr, mr, det[s], got, 3 * X.CHUNKS - 3)
    assert moved >= 200, moved


# ---------------------------------------------------------------------------------------------- 5. refusals

def test_refusals(ra, ctx, banks, pcm):
    cfg = config(ra, X.Cfg())
    sb = batch(ra, ctx, banks, cfg)
    part = np.ascontiguousarray(pcm[:, :960])
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_logits: the streams have not received audio yet"):
        sb.logits()
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_slot_scores: the streams have not received audio yet"):
        sb.slot_scores()
    with pytest.raises(ra.RustpotterError, match="a batch over mixed sets has no single aggregate per window"):
        sb.process(part, want_agg=True)
    det, n_det = sb.process(part)      # without agg it works
    assert not n_det.any() and sb.chunks_seen == 2
    one = np.zeros(X.S, np.int32)
    for call, text in ((lambda: sb.set_wakewords(0, one), "rp_stream_batch_set_wakewords: the batch runs over mixed sets"),
                       (lambda: sb.set_wakeword_sets(0, X.REF_ROWS), "rp_stream_batch_set_wakeword_sets: the batch runs over mixed sets"),
                       (lambda: sb.set_models(0, one), "rp_stream_batch_set_models: the batch runs over mixed sets"),
                       (lambda: sb.set_model_sets(0, X.MODEL_ROWS), "rp_stream_batch_set_model_sets: the batch runs over mixed sets")):
        with pytest.raises(ra.RustpotterError, match=text):
            call()
    sb.reset(0)
    sb.reset(-1)
    f = ra.FiltersConfig()
    f.gain_normalizer.enabled = True
    fresh = batch(ra, ctx, banks, cfg)
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_filters: the gain normaliser is not available on a batch over mixed sets"):
        fresh.set_filters(f)
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_filters_bank: a batch over mixed sets"):
        fresh.set_filters_bank(f)
    band = ra.FiltersConfig()
    band.band_pass.enabled = True
    fresh.set_filters(band)            # the band-pass alone works
    fresh.process_multi(part)
    # 48 kHz input: the front stages are those of every live batch
    a = batch(ra, ctx, banks, cfg, sample_rate=48000)
    assert a.samples_per_chunk == 1440
    a.process_multi(np.repeat(part, 3, axis=1))
    # the other kinds refuse the new call
    sets = ra.StreamBatch(ctx, None, cfg, X.S, max_chunks_per_call=2, bank=banks[0], stream_wakewords=X.REF_ROWS)
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_mixed_sets: the batch was not made by rp_stream_batch_new_mixed_sets"):
        sets.set_mixed_sets(0, X.REF_ROWS, X.MODEL_ROWS)
    # creation: set sizes, indices (before anything is allocated), the mfcc_size rule, a foreign context
    with pytest.raises(ra.RustpotterError, match=r"ref_set_size 9 is outside 0 \.\. 8"):
        batch(ra, ctx, banks, cfg, ref_rows=np.full((X.S, 9), -1, np.int32))
    with pytest.raises(ra.RustpotterError, match=r"model_set_size 9 is outside 0 \.\. 8"):
        batch(ra, ctx, banks, cfg, model_rows=np.full((X.S, 9), -1, np.int32))
    bad = X.MODEL_ROWS.copy()
    bad[7, 1] = banks[1].W
    with pytest.raises(ra.RustpotterError, match="stream 7, slot 1: model index"):
        batch(ra, ctx, banks, cfg, model_rows=bad)
    five = ra.WakewordBank(ctx, wakewords=[([orc.synth_templates(3, 1, 40, 5)[0]], None, None, None)])
    with pytest.raises(ra.RustpotterError, match="Usage of wakewords with different mfcc size is not supported"):
        batch(ra, ctx, (five, banks[1]), cfg)
    other = ra.BatchContext(device=0, host_pointers=True)
    with pytest.raises(ra.RustpotterError, match="the wakeword bank belongs to another context"):
        batch(ra, other, banks, cfg)
    # two empty banks: calls succeed and report nothing
    ebanks = (ra.WakewordBank(ctx, wakewords=[]), ra.ModelBank(ctx, models=[]))
    none = np.full((X.S, 2), -1, np.int32)
    eb = batch(ra, ctx, ebanks, cfg, ref_rows=none, model_rows=none)
    det, dww, dlab, n_det = eb.process_multi(part)
    assert not n_det.any()
    # one side absent (a size of 0): the other side's detections
    only = ra.StreamBatch(ctx, None, cfg, X.S, max_chunks_per_call=MAX_CHUNKS, bank=banks[0], stream_wakewords=X.REF_ROWS, model_bank=banks[1],
                          stream_models=None)
    assert only.model_set_size == 0 and only.set_size == 2
    got, _ = feed(only, pcm, (10,))
    sets = ra.StreamBatch(ctx, None, cfg, X.S, max_chunks_per_call=MAX_CHUNKS, bank=banks[0], stream_wakewords=X.REF_ROWS)
    n = 0
    for c0 in range(0, X.CHUNKS, 10):
        d, w, lab, nd = sets.process_multi(np.ascontiguousarray(pcm[:, c0 * 480:(c0 + 10) * 480]), max_det=MAX_CHUNKS + 1)
        n += int(nd.sum())
    assert n == sum(len(v) for v in got) and n >= 5
