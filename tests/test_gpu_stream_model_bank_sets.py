"""Model sets on live streams: a live-stream batch in which stream s holds a set of models of a model bank
(rp_stream_batch_new_model_bank_sets / _set_model_sets / _logits; window_means_set_stream_kernel, mlp_set_stream_kernel,
nn_score_set_stream_kernel, scan_model_set_stream_kernel).  The first window of a call starts Lmax(s) - 1 frames before the first new frame
for every slot and slot j reads L_j frames from there, row by row with the arithmetic of mlp_mfma_kernel's three-part form -- so the
yardsticks hold BIT FOR BIT: any other cut of the audio into calls, rp_mlp_forward_windows over fewer than 32 windows at the shifted
position, and the shared-model live batch (rp_stream_batch_new_multi) with the live slots' models as its wakewords.  Against the
whole-recording sets call over the concatenation: equal detections, scores within 2e-6 (the figure for this pair of
kernels).  Calls of 1, 6 and 11 chunks: one partial 16-row tile, two tiles with the second partial, a second wave per slot.
Bank, rows and audio: tests/model_set_cases.py."""
import numpy as np
import pytest

import model_set_cases as M

pytestmark = pytest.mark.gpu
MAX_CHUNKS = 11
IN_PLACE = "mlp_mfma_kernel<bf16x3 splits>"
# (threshold, avg_threshold, vad, eager, min_scores)
CONFIGS = [(M.THRESHOLD, 0.0, None, False, 1), (M.THRESHOLD, M.AVG_THRESHOLD, None, True, 2), (M.THRESHOLD, 0.0, "easy", False, 1)]


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


@pytest.fixture(scope="module")
def weights():
    return M.bank_weights()


@pytest.fixture(scope="module")
def models(ra, ctx, weights):
    return [ra.Model(ctx, ws, bs) for ws, bs in weights]


@pytest.fixture(scope="module")
def bank(ra, ctx, models):
    return ra.ModelBank(ctx, models=models, none_index=M.NONE_INDEX)


@pytest.fixture(scope="module")
def pcm():
    return M.pcm().astype(np.float32)


def config(ra, threshold, avg_threshold, vad, eager, min_scores):
    cfg = ra.DetectorConfig()
    cfg.threshold, cfg.avg_threshold, cfg.eager, cfg.min_scores = threshold, avg_threshold, eager, min_scores
    if vad:
        cfg.vad_mode = ra.VADMode.Easy
    return cfg


def f32(b):
    return float(np.array([b], np.uint32).view(np.float32)[0])


def feed(sb, pcm, pieces, want_logits=True, before_chunk=None, chunk=480):
    """pcm [S][C * chunk] through the batch in calls of pieces[0], pieces[1], ... chunks (cycled) -> per stream the list of (frame, window,
    counter, score bits, avg bits, wakeword, label), and the logits of every call side by side along the frame axis"""
    n_streams, total = pcm.shape[0], pcm.shape[1] // chunk
    out, logits = [[] for _ in range(n_streams)], []
    c = k = 0
    while c < total:
        n = min(pieces[k % len(pieces)], total - c)
        k += 1
        if before_chunk is not None:
            before_chunk(c)
        det, dww, dlab, n_det = sb.process_multi(np.ascontiguousarray(pcm[:, c * chunk:(c + n) * chunk]), max_det=MAX_CHUNKS + 1)
        for s in range(n_streams):
            for i in range(n_det[s]):
                d = det[s][i]
                assert d["stream"] == s
                out[s].append((int(d["frame"]), int(d["window"]), int(d["counter"]), M.bits(d["score"]), M.bits(d["avg_score"]), int(dww[s][i]),
                               int(dlab[s][i])))
            assert not det[s][n_det[s]:].tobytes().strip(b"\0") and (dlab[s][n_det[s]:] == -1).all()
        if want_logits:
            logits.append(sb.logits())
        c += n
    assert sb.chunks_seen == total
    return out, (np.concatenate(logits, axis=-2) if want_logits else None)


def live(ra, ctx, bank, pcm, sets, pieces, cfg=None, **kw):
    sets = np.asarray(sets, np.int32)
    sb = ra.StreamBatch(ctx, None, cfg or config(ra, *CONFIGS[1]), len(sets), max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_models=sets)
    return feed(sb, pcm, pieces, **kw)


def same_logits(a, b, sets):
    """windows that lie inside the audio: column j is the window that ends at frame j - 3 and starts Lmax(s) - 1 frames before it"""
    for s, row in enumerate(sets):
        first = max(M.lmax_of(row) - 1, 0) + 3
        x, y = a[s, :, first:], b[s, :, first:]
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), (s, int(np.sum(x.view(np.uint32) != y.view(np.uint32))))


@pytest.fixture(scope="module")
def one_chunk(ra, ctx, bank, pcm):
    """the reference run: calls of one chunk (one partial row tile)"""
    det, lg = live(ra, ctx, bank, pcm, M.SETS, (1,))
    assert lg.shape == (M.S, M.SET_SIZE, 3 * M.CHUNKS, M.LABEL_PITCH)
    print("calls of 1 chunk: %s detections" % [len(d) for d in det])
    assert sum(len(d) for d in det) >= 15 and not det[4]
    return det, lg


@pytest.mark.parametrize("pieces", [(6,), (11,), (3, 1, 2)])
def test_call_cut_invariance(ra, ctx, bank, pcm, one_chunk, pieces):
    """the same audio in other calls: the logits of every window and the detections are those of the 1-chunk run, bit for bit"""
    det, lg = live(ra, ctx, bank, pcm, M.SETS, pieces)
    assert det == one_chunk[0]
    same_logits(lg, one_chunk[1], M.SETS)


def test_logits_bit_for_bit(ctx, models, pcm, one_chunk):
    """slot j of stream s over runs of fewer than 32 consecutive frames against rp_mlp_forward_windows over the L_j-frame windows that start
    where the set's windows start: equal bits; zeros behind the labels and in empty slots"""
    _, lg = one_chunk
    mfcc = ctx.mfcc(pcm, M.K)
    n_live = lg.shape[2] - 3   # frames 0 .. n_live - 1 have been seen
    compared = 0
    for s, row in enumerate(M.SETS):
        lm = M.lmax_of(row)
        for j, mi in enumerate(row):
            if mi < 0:
                assert not lg[s, j].any(), (s, j)
                continue
            L, nl = M.MODELS[mi][0], M.MODELS[mi][2]
            assert not lg[s, j, :, nl:].any(), (s, j)
            for f0, n in ((lm - 1, 31), (lm - 1 + 31, 7), (n_live - 20, 20)):
                w0 = f0 - lm + 1   # the frame the window that ends at f0 starts at
                want = ctx.mlp_forward_windows(mfcc[s:s + 1, w0:w0 + n - 1 + L], models[mi])[0]
                assert ctx.last_mlp_kernel().startswith(IN_PLACE), ctx.last_mlp_kernel()
                got = lg[s, j, f0 + 3:f0 + 3 + n, :nl]
                assert want.shape == (n, nl) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (s, j, mi, f0, n)
                compared += n
    print("%d windows compared" % compared)
    assert compared == int((M.SETS >= 0).sum()) * 58


@pytest.mark.parametrize("case", range(len(CONFIGS)))
def test_against_the_whole_recording(ra, ctx, bank, pcm, case):
    """rp_batch_detect_model_bank_sets over the concatenation: equal frame, window, counter, bank index and label, scores within 2e-6"""
    cfg = config(ra, *CONFIGS[case])
    det, _ = live(ra, ctx, bank, pcm, M.SETS, (6,), cfg=cfg, want_logits=False)
    wdet, wmod, wlab, wn = ctx.batch_detect_model_bank_sets(pcm, bank, M.SETS, cfg, max_det=32)
    last = 3 * M.CHUNKS - 4   # the last frame the live streams have seen
    total, worst = 0, 0.0
    for s in range(M.S):
        want = [(int(d["frame"]), int(d["window"]), int(d["counter"]), float(d["score"]), float(d["avg_score"]), int(wmod[s][j]), int(wlab[s][j]))
                for j, d in enumerate(wdet[s][:wn[s]]) if d["frame"] <= last]
        assert [d[:3] + d[5:] for d in det[s]] == [w[:3] + w[5:] for w in want], (s, det[s], want)
        for d, w in zip(det[s], want):
            worst = max(worst, abs(f32(d[3]) - w[3]), abs(f32(d[4]) - w[4]))
        total += len(want)
    print("case %d: %d detections, worst score difference %.3g" % (case, total, worst))
    assert worst <= 2e-6
    if CONFIGS[case][2] is None:
        assert total >= 15


def test_against_the_shared_model_live_batch(ra, ctx, models, pcm, one_chunk):
    """per stream: rp_stream_batch_new_multi on the stream alone with its live slots' models as wakewords, calls of at most 10 chunks --
    every detection equal, score and avg bits, the winner (slot -> bank index) and the label included"""
    cfg = config(ra, *CONFIGS[1])
    seen = 0
    for s, row in enumerate(M.SETS):
        live_slots = [int(mi) for mi in row if mi >= 0]
        if not live_slots:
            continue
        specs = [{"model": models[mi], "none_index": M.NONE_INDEX[mi]} for mi in live_slots]
        sb = ra.StreamBatch(ctx, None, cfg, 1, max_chunks_per_call=10, wakewords=specs, mfcc_size=M.K)
        det, _ = feed(sb, pcm[s:s + 1], (10, 3, 1), want_logits=False)
        want = [d[:5] + (live_slots[d[5]], d[6]) for d in det[0]]
        assert want == one_chunk[0][s], (s, want, one_chunk[0][s])
        seen += len(want)
    assert seen >= 15


def test_set_size_one_equals_the_model_bank_batch(ra, ctx, bank, pcm):
    idx = np.array([0, 3, 1, -1, 2, 4, 5, 1, 0], np.int32)
    cfg = config(ra, *CONFIGS[1])
    det, lg = live(ra, ctx, bank, pcm, idx[:, None], (6, 1))
    sb = ra.StreamBatch(ctx, None, cfg, M.S, max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_model=idx)
    wdet, wlg = feed(sb, pcm, (6, 1))
    assert det == wdet and sum(len(d) for d in det) >= 10
    assert lg.shape == (M.S, 1) + wlg.shape[1:] and np.array_equal(lg[:, 0].view(np.uint32), wlg.view(np.uint32))


def test_set_model_sets_reset_and_a_refused_row(ra, ctx, bank, pcm, one_chunk):
    """re-targeting at chunk 40: the streams behave from there as streams that were reset then (rp_stream_batch_reset at the same chunk on a
    batch that held the new rows from the start); a refused row changes nothing"""
    cfg = config(ra, *CONFIGS[1])
    new_rows = np.array([[2, -1, 0], [0, 5, 1]], np.int32)
    sets = M.SETS.copy()
    sb = ra.StreamBatch(ctx, None, cfg, M.S, max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_models=sets)

    def retarget(c):
        if c == 40:
            bad = new_rows.copy()
            bad[1, 2] = bank.W
            with pytest.raises(ra.RustpotterError, match="stream 3, slot 2"):
                sb.set_model_sets(2, bad)
            sb.set_model_sets(2, new_rows)
    det, _ = feed(sb, pcm, (4,), want_logits=False, before_chunk=retarget)
    sets[2:4] = new_rows
    ref = ra.StreamBatch(ctx, None, cfg, M.S, max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_models=sets)

    def reset(c):
        if c == 40:
            ref.reset(2)
            ref.reset(3)
    want, _ = feed(ref, pcm, (4,), want_logits=False, before_chunk=reset)
    for s in range(M.S):
        if s in (2, 3):
            assert [d for d in det[s] if d[0] >= 120] == [d for d in want[s] if d[0] >= 120], s
            assert [d for d in det[s] if d[0] < 117] == [d for d in one_chunk[0][s] if d[0] < 117], s
        else:
            assert det[s] == want[s] == one_chunk[0][s], s
    assert any(d[0] >= 120 for d in det[2] + det[3])


def test_resampled_input_and_band_pass(ra, ctx, bank, pcm):
    """48 kHz input and the band-pass filter: the front stages are those of every live batch; a sets batch over rows of one live slot gives
    the detections and logits of the model-bank batch fed the same"""
    idx = np.array([0, 3, 1, -1, 2, 4, 5, 1, 0], np.int32)
    cfg = config(ra, *CONFIGS[1])
    x48 = np.repeat(pcm[:, :480 * 60], 3, axis=1)
    a = ra.StreamBatch(ctx, None, cfg, M.S, max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_models=idx[:, None], sample_rate=48000)
    b = ra.StreamBatch(ctx, None, cfg, M.S, max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_model=idx, sample_rate=48000)
    assert a.samples_per_chunk == 1440
    da, la = feed(a, x48, (6,), chunk=1440)
    db, lb = feed(b, x48, (6,), chunk=1440)
    assert da == db and np.array_equal(la[:, 0].view(np.uint32), lb.view(np.uint32))
    f = ra.FiltersConfig()
    f.band_pass.enabled = True
    a = ra.StreamBatch(ctx, None, cfg, M.S, max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_models=M.SETS, filters=f)
    b = ra.StreamBatch(ctx, None, cfg, M.S, max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_models=M.SETS, filters=f)
    da, la = feed(a, pcm[:, :480 * 60], (6,))
    db, lb = feed(b, pcm[:, :480 * 60], (1,))
    assert da == db
    same_logits(la, lb, M.SETS)


def test_put_under_the_batch(ra, ctx, weights, pcm):
    """a put that lengthens a stream's Lmax within the reservation is read in the next call; one beyond it is refused"""
    short = [ra.Model(ctx, *weights[i]) for i in (0, 1)]
    bk = ra.ModelBank(ctx, models=short, none_index=[0, 0])
    bk.reserve(max_train_size=96, max_labels=3)
    cfg = config(ra, *CONFIGS[1])
    sets = np.array([[0, 1, -1], [1, -1, -1]], np.int32)
    sb = ra.StreamBatch(ctx, None, cfg, 2, max_chunks_per_call=MAX_CHUNKS, model_bank=bk, stream_models=sets)

    def grow(c):
        if c == 42:
            bk.put(1, [ra.Model(ctx, *weights[2])], none_index=[M.NONE_INDEX[2]])     # index 1: L 47 -> 96
            with pytest.raises(ra.RustpotterError, match="195"):
                bk.put(0, [ra.Model(ctx, *weights[3])], none_index=[0])
            sb.set_model_sets(0, sets)   # add_wakeword on the detectors: a reset, as the reference does
    det, _ = feed(sb, pcm[:2], (6,), want_logits=False, before_chunk=grow)
    # the yardstick: a bank that held the long model from the start, the streams reset at the same chunk
    bk2 = ra.ModelBank(ctx, models=[short[0], ra.Model(ctx, *weights[2])], none_index=[0, M.NONE_INDEX[2]])
    ref = ra.StreamBatch(ctx, None, cfg, 2, max_chunks_per_call=MAX_CHUNKS, model_bank=bk2, stream_models=sets)
    want, _ = feed(ref, pcm[:2], (6,), want_logits=False, before_chunk=lambda c: ref.reset(-1) if c == 42 else None)
    for s in range(2):
        after = [d for d in det[s] if d[0] >= 126]
        assert after == [d for d in want[s] if d[0] >= 126], (s, det[s], want[s])
        assert all(126 <= d[1] <= d[0] - 96 for d in after)   # windows of the new Lmax, 96 frames, none reaching before the reset
    assert sum(1 for s in range(2) for d in det[s] if d[0] >= 126) >= 2
    sb.close()
    ref.close()


def test_refusals(ra, ctx, bank, pcm):
    cfg = config(ra, *CONFIGS[0])
    sb = ra.StreamBatch(ctx, None, cfg, M.S, max_chunks_per_call=2, model_bank=bank, stream_models=M.SETS)
    part = np.ascontiguousarray(pcm[:, :960])
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_logits: the streams have not received audio yet"):
        sb.logits()
    with pytest.raises(ra.RustpotterError, match="no aggregate per window"):
        sb.process(part, want_agg=True)
    det, n_det = sb.process(part)      # without agg it works
    assert not n_det.any()
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_models: the batch holds model sets"):
        sb.set_models(0, np.zeros(M.S, np.int32))
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_wakewords: the batch runs over model sets"):
        sb.set_wakewords(0, np.zeros(M.S, np.int32))
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_wakeword_sets: the batch runs over model sets"):
        sb.set_wakeword_sets(0, M.SETS)
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_slot_scores: a batch over model sets"):
        sb.slot_scores()
    with pytest.raises(ra.RustpotterError, match="streams 8 .. 8 \\+ 2 reach past the batch's 9 streams"):
        sb.set_model_sets(8, M.SETS[:2])
    f = ra.FiltersConfig()
    f.gain_normalizer.enabled = True
    fresh = ra.StreamBatch(ctx, None, cfg, M.S, max_chunks_per_call=2, model_bank=bank, stream_models=M.SETS)
    with pytest.raises(ra.RustpotterError, match="gain normaliser is not available on a batch over a model bank"):
        fresh.set_filters(f)
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_filters_bank: the gain normaliser per model is not built"):
        fresh.set_filters_bank(f)
    # the other kinds refuse the new call
    one = ra.StreamBatch(ctx, None, cfg, M.S, max_chunks_per_call=2, model_bank=bank, stream_model=np.zeros(M.S, np.int32))
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_model_sets: the batch was not made by rp_stream_batch_new_model_bank_sets"):
        one.set_model_sets(0, M.SETS)
    # creation: set_size, indices (before anything is allocated), a foreign context
    with pytest.raises(ra.RustpotterError, match="RP_MODEL_SET_MAX"):
        ra.StreamBatch(ctx, None, cfg, M.S, model_bank=bank, stream_models=np.full((M.S, 9), -1, np.int32))
    bad = M.SETS.copy()
    bad[7, 1] = bank.W
    with pytest.raises(ra.RustpotterError, match="stream 7, slot 1: model index"):
        ra.StreamBatch(ctx, None, cfg, M.S, model_bank=bank, stream_models=bad)
    other = ra.BatchContext(device=0, host_pointers=True)
    with pytest.raises(ra.RustpotterError, match="the bank belongs to another context"):
        ra.StreamBatch(other, None, cfg, M.S, model_bank=bank, stream_models=M.SETS)
    # an empty bank: calls succeed and report nothing
    empty = ra.ModelBank(ctx, models=[])
    eb = ra.StreamBatch(ctx, None, cfg, M.S, max_chunks_per_call=2, model_bank=empty, stream_models=np.full((M.S, 2), -1, np.int32))
    det, dww, dlab, n_det = eb.process_multi(part)
    assert not n_det.any()
