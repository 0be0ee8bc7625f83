"""Personal wakeword models on live streams: a live-stream batch over a model bank (rp_stream_batch_new_model_bank / _set_models / _logits;
mlp_bank_stream_kernel, window_means_bank_stream_kernel, nn_score_bank_stream_kernel, scan_bank_stream_kernel with labels).  Stream s runs
its own model bank[stream_model[s]] and is fed chunk by chunk.  The kernel computes every window row by row with the arithmetic of
mlp_mfma_kernel's three-part form reading the window in place with its own mean, so the yardsticks hold BIT FOR BIT: rp_mlp_forward_windows
over fewer than 32 windows of rp_mfcc_batch's rows, any other cut of the same audio into calls, any other batch, and the shared-model live
batch (rp_stream_batch_new_multi) with the stream's model.  Against the whole-recording bank call (mlp_windows_bank_kernel: frames staged
relative to a workgroup's middle window) detections are equal and scores within 2e-6, the project's figure for that pair of kernels; against
the CPU oracle's detector the parity bar, 1e-5.
The six models, STREAM_MODEL (S = 13, one stream without a model) and the detection set-up are those of tests/test_gpu_model_bank.py: L of
30 / 75 / 195 / 256 (odd L: 16 L is no multiple of 32; L = 75: no multiple of 128), widths of 2 to 32, two and three layers, a model
without "none"; on 3 s of rp_synth_pcm_batch noise 5 streams fire and no score lies within 2e-3 of the threshold."""
import numpy as np
import pytest

from oracle import rp_oracle as orc
from test_gpu_model_bank import (DET_GAIN, DET_MODEL_SEED, DET_SEED, DET_THRESHOLD, K, MODELS, NONE_INDEX, STREAM_MODEL, S, bank_weights,
                                 model_dict)

pytestmark = pytest.mark.gpu
CHUNKS = 100           # 3 s
MAX_CHUNKS = 11        # a call of 11 chunks has 33 rows: past two 16-row tiles and past the 32 at which the shared path changes kernel
IN_PLACE = "mlp_mfma_kernel<bf16x3 splits>"


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


@pytest.fixture(scope="module")
def pcm(ctx):
    return ctx.synth_pcm(DET_SEED, 0, S, 480 * CHUNKS)


@pytest.fixture(scope="module")
def weights():
    return bank_weights(DET_MODEL_SEED, DET_GAIN)


@pytest.fixture(scope="module")
def models(ra, ctx, weights):
    return [ra.Model(ctx, ws, bs) for ws, bs in weights]


@pytest.fixture(scope="module")
def bank(ra, ctx, models):
    return ra.ModelBank(ctx, models=models, none_index=NONE_INDEX)


def config(ra, avg_threshold=0.0, vad=None):
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold, cfg.min_scores = avg_threshold, DET_THRESHOLD, 1
    if vad:
        cfg.vad_mode = ra.VADMode.Easy
    return cfg


def bits1(x):
    return int(np.float32(x).view(np.uint32))


def f32(b):
    return float(np.array([b], np.uint32).view(np.float32)[0])


def feed(sb, pcm, pieces, before_chunk=None, want_logits=True, multi=True):
    """pcm [S][C * 480] through the batch in calls of pieces[0], pieces[1], ... chunks (cycled) -> per stream the list of (frame, window,
    counter, score bits, avg bits, model index, label), and the logits of every call side by side, [S][3 C][label pitch]: column j is the
    window that ends at frame j - 3.  before_chunk(c): called between calls, before the chunk with index c is fed."""
    n_streams, total = pcm.shape[0], pcm.shape[1] // 480
    out, logits = [[] for _ in range(n_streams)], []
    c = k = 0
    while c < total:
        n = min(pieces[k % len(pieces)], total - c)
        k += 1
        if before_chunk is not None:
            before_chunk(c)
        part = np.ascontiguousarray(pcm[:, c * 480:(c + n) * 480])
        if multi:
            det, dww, dlab, n_det = sb.process_multi(part, max_det=MAX_CHUNKS + 1)
        else:
            det, n_det = sb.process(part, max_det=MAX_CHUNKS + 1)
            dww = dlab = None
        for s in range(n_streams):
            assert n_det[s] <= MAX_CHUNKS
            for i in range(n_det[s]):
                d = det[s][i]
                assert d["stream"] == s
                out[s].append((int(d["frame"]), int(d["window"]), int(d["counter"]), bits1(d["score"]), bits1(d["avg_score"]),
                               None if dww is None else int(dww[s][i]), None if dlab is None else int(dlab[s][i])))
            assert not det[s][n_det[s]:].tobytes().strip(b"\0"), "slots behind a stream's detections are zero"
            if dlab is not None:
                assert (dlab[s][n_det[s]:] == -1).all()
        if want_logits:
            lg = sb.logits()
            assert lg.shape[:2] == (n_streams, 3 * n)
            logits.append(lg)
        c += n
    assert sb.chunks_seen == total
    return out, (np.concatenate(logits, axis=1) if want_logits else None)


def live(ra, ctx, bank, pcm, idx, pieces, cfg=None, **kw):
    sb = ra.StreamBatch(ctx, None, cfg or config(ra), len(idx), max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_model=np.asarray(idx, np.int32))
    return feed(sb, pcm, pieces, **kw)


def full_windows(lg, idx):
    """per stream the logits of the windows that lie inside the audio: frames L - 1 .. (column frame + 3)"""
    return [lg[s, MODELS[mi][1] - 1 + 3:] if mi >= 0 else lg[s] for s, mi in enumerate(idx)]


def same_logits(a, b, idx):
    for s, (x, y) in enumerate(zip(full_windows(a, idx), full_windows(b, idx))):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), (s, int(np.sum(x.view(np.uint32) != y.view(np.uint32))))


@pytest.fixture(scope="module")
def one_chunk(ra, ctx, bank, pcm):
    """the reference run: calls of one chunk"""
    det, lg = live(ra, ctx, bank, pcm, STREAM_MODEL, (1,))
    fired = sum(1 for d in det if d)
    print("calls of 1 chunk: %d of 12 streams fire, %s detections" % (fired, [len(d) for d in det]))
    assert fired == 5 and not det[3]
    for s, mi in enumerate(STREAM_MODEL):
        assert all(d[5] == mi and 0 <= d[6] < len(MODELS[mi][3]) and d[6] != NONE_INDEX[mi] for d in det[s]), (s, det[s])
    return det, lg


def test_logits_bit_for_bit(ctx, models, pcm, one_chunk):
    """windows that end at runs of fewer than 32 consecutive frames -- the stream's first full window on, and the last of the audio -- against
    rp_mlp_forward_windows over exactly those frames of rp_mfcc_batch's rows with the stream's own rp_model: equal bits, zeros behind the labels"""
    _, lg = one_chunk
    mfcc = ctx.mfcc(pcm, K)
    n_live = lg.shape[1] - 3   # frames 0 .. n_live - 1 have been seen
    assert lg.shape == (S, 3 * CHUNKS, 3) and mfcc.shape[1] >= n_live
    compared = 0
    for s, mi in enumerate(STREAM_MODEL):
        if mi < 0:
            assert not lg[s].any()
            continue
        L, nl = MODELS[mi][1], len(MODELS[mi][3])
        assert not lg[s, :, nl:].any(), s
        for f0, n in ((L - 1, 31), (L - 1 + 31, 7), (n_live - 20, 20)):
            if f0 + n > n_live:
                n = n_live - f0
            want = ctx.mlp_forward_windows(mfcc[s:s + 1, f0 - L + 1:f0 + n], models[mi])[0]
            assert ctx.last_mlp_kernel().startswith(IN_PLACE), ctx.last_mlp_kernel()
            got = lg[s, f0 + 3:f0 + 3 + n, :nl]
            assert want.shape == (n, nl) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (s, mi, f0, n)
            compared += n
    print("%d windows compared" % compared)
    assert compared >= 12 * 40


@pytest.mark.parametrize("pieces", [(8,), (3, 1, 2), (11,)])
def test_call_cut_invariance(ra, ctx, bank, pcm, one_chunk, pieces):
    """the same audio in other calls: the logits of every window and the detections are those of the 1-chunk run, bit for bit"""
    det, lg = live(ra, ctx, bank, pcm, STREAM_MODEL, pieces)
    assert det == one_chunk[0]
    same_logits(lg, one_chunk[1], STREAM_MODEL)


def test_batch_invariance(ra, ctx, bank, pcm, one_chunk):
    """a stream alone in a batch of S = 1, and the same streams in another order, give the same bits"""
    perm = np.random.default_rng(1).permutation(S)
    det, lg = live(ra, ctx, bank, pcm[perm], STREAM_MODEL[perm], (3, 1, 2))
    assert det == [one_chunk[0][p] for p in perm]
    same_logits(lg, one_chunk[1][perm], STREAM_MODEL[perm])
    for s in (0, 1, 5, 6):
        det, lg = live(ra, ctx, bank, pcm[s:s + 1], STREAM_MODEL[s:s + 1], (11,))
        assert det == [one_chunk[0][s]]
        same_logits(lg, one_chunk[1][s:s + 1], STREAM_MODEL[s:s + 1])


def test_against_the_shared_model_live_batch(ra, ctx, models, pcm, one_chunk):
    """per stream with a model: rp_stream_batch_new_multi with that one model, fed the same audio in calls of at most 10 chunks -- every
    detection equal, score and avg bits and the label included"""
    cfg = config(ra)
    for s, mi in enumerate(STREAM_MODEL):
        if mi < 0:
            continue
        sb = ra.StreamBatch(ctx, None, cfg, 1, max_chunks_per_call=10, wakewords=[{"model": models[mi], "none_index": NONE_INDEX[mi]}], mfcc_size=K)
        det, _ = feed(sb, pcm[s:s + 1], (10, 3, 1), want_logits=False)
        assert [d[:5] + d[6:] for d in det[0]] == [d[:5] + d[6:] for d in one_chunk[0][s]], (s, mi, det[0], one_chunk[0][s])


@pytest.mark.parametrize("avg_threshold,vad", [(0.0, None), (0.2, None), (0.0, "easy")])
def test_against_the_whole_recording(ra, ctx, bank, pcm, avg_threshold, vad):
    """rp_batch_detect_model_bank over the concatenation: equal frame, window, counter and label, scores within 2e-6 (INTEGRATION.md section 3:
    mlp_windows_bank_kernel against the row's own mean)"""
    cfg = config(ra, avg_threshold, vad)
    det, _ = live(ra, ctx, bank, pcm, STREAM_MODEL, (8,), cfg=cfg, want_logits=False)
    wdet, wlab, wn = ctx.batch_detect_model_bank(pcm, bank, STREAM_MODEL, cfg, max_det=32)
    last = 3 * CHUNKS - 4   # the last frame the live streams have seen
    fired, worst = 0, 0.0
    for s in range(S):
        want = [(int(d["frame"]), int(d["window"]), int(d["counter"]), float(d["score"]), float(d["avg_score"]), int(wlab[s][j]))
                for j, d in enumerate(wdet[s][:wn[s]]) if d["frame"] <= last]
        assert [d[:3] + (d[6],) for d in det[s]] == [w[:3] + (w[5],) for w in want], (s, det[s], want)
        for d, w in zip(det[s], want):
            worst = max(worst, abs(f32(d[3]) - w[3]), abs(f32(d[4]) - w[4]))
        fired += bool(want)
    print("avg_threshold %g vad %s: %d streams fire, worst score difference %.3g" % (avg_threshold, vad, fired, worst))
    assert worst <= 2e-6
    assert fired == (0 if vad else 5)


def test_against_the_oracle(ra, weights, pcm, one_chunk):
    """oracle.rp_oracle.Detector.add_model per stream, fed the same chunks: detections exact (chunk, counter, label), scores within 1e-5"""
    worst, n = 0.0, 0
    for s, mi in enumerate(STREAM_MODEL):
        if mi < 0:
            continue
        d = orc.Detector(avg_threshold=0.0, threshold=DET_THRESHOLD, min_scores=1)
        d.add_model(model_dict(mi, *weights[mi]))
        want = [(i // 480, r) for i in range(0, pcm.shape[1] - 479, 480) for r in [d.process_f32(pcm[s, i:i + 480])] if r is not None]
        got = one_chunk[0][s]
        assert len(got) == len(want), (s, got, want)
        for g, (chunk, r) in zip(got, want):
            assert g[0] // 3 + 1 == chunk and g[2] == r["counter"] and MODELS[mi][3][g[6]] == r["name"], (s, g, chunk, r)
            worst = max(worst, abs(f32(g[3]) - float(r["score"])), abs(f32(g[4]) - float(r["avg_score"])))
            n += 1
    print("%d detections, worst score difference against the oracle %.3g" % (n, worst))
    assert n >= 5 and worst <= 1e-5


def test_set_models(ra, ctx, bank, pcm, one_chunk):
    """after 20 chunks: one stream disconnected, one retarget to a model of another window length, the stream without a model connected
    (the two hear the audio of streams that fire with those models).  From there a touched stream equals a fresh batch started at that chunk
    with that model; before, the run it had; untouched streams equal the uninterrupted run, bit for bit; a refused index names its stream and
    changes nothing"""
    half = 20
    idx = STREAM_MODEL.copy()
    new = {1: -1, 4: 2, 3: 0}   # stream 1 (L 30) off; stream 4: model 1 (L 195) -> model 2 (L 75); stream 3: none -> model 0 (L 30)
    assert all(idx[s] != m for s, m in new.items()) and MODELS[idx[4]][1] != MODELS[2][1] and idx[6] == 2 and idx[7] == 0
    pcm = pcm.copy()
    pcm[4], pcm[3] = pcm[6], pcm[7]
    sb = ra.StreamBatch(ctx, None, config(ra), S, max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_model=idx)

    def at(c):
        if c != half:
            return
        with pytest.raises(ra.RustpotterError, match="stream 3"):
            sb.set_models(2, np.array([0, bank.W], np.int32))
        with pytest.raises(ra.RustpotterError, match="reach past"):
            sb.set_models(S - 1, np.array([0, 0], np.int32))
        sb.set_models(1, np.array([new[1]], np.int32))
        sb.set_models(3, np.array([new[3], new[4]], np.int32))

    det, lg = feed(sb, pcm, (5,), before_chunk=at)
    touched = 0
    for s in range(S):
        if s not in new:
            assert det[s] == one_chunk[0][s], s
            same_logits(lg[s:s + 1], one_chunk[1][s:s + 1], idx[s:s + 1])
            continue
        # before the change: the run the stream had with its old model; no detection is reported across the change (the stream was reset)
        old = idx[s:s + 1]
        bdet, blg = live(ra, ctx, bank, pcm[s:s + 1, :half * 480], old, (5,))
        assert [d for d in det[s] if d[0] < 3 * half - 3] == bdet[0], s
        same_logits(lg[s:s + 1, :3 * half], blg, old)
        mi = new[s]
        if mi < 0:
            assert not [d for d in det[s] if d[0] >= 3 * half - 3] and not lg[s, 3 * half:].any()
            continue
        fdet, flg = live(ra, ctx, bank, pcm[s:s + 1, half * 480:], [mi], (5,))
        moved = [(d[0] + 3 * half, d[1] + 3 * half) + d[2:] for d in fdet[0]]
        assert [d for d in det[s] if d[0] >= 3 * half - 3] == moved, (s, det[s], moved)
        same_logits(lg[s:s + 1, 3 * half:], flg, [mi])
        touched += len(moved)
    print("detections of the touched streams after the change: %d" % touched)
    assert touched >= 2


def test_refusals_and_edges(ra, ctx, bank, models, pcm, one_chunk):
    cfg = config(ra)
    part = np.ascontiguousarray(pcm[:, :480 * 2])
    sb = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=2, model_bank=bank, stream_model=STREAM_MODEL)
    with pytest.raises(ra.RustpotterError, match="not received audio"):
        sb.logits()
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_logits"):
        sb.process(part, want_agg=True)
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_models"):
        sb.set_wakewords(0, np.zeros(1, np.int32))
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_models"):
        sb.set_wakeword_sets(0, np.zeros((1, 1), np.int32))
    with pytest.raises(ra.RustpotterError, match="over a model bank"):
        sb.slot_scores()
    gain = ra.FiltersConfig()
    gain.gain_normalizer.enabled = True
    with pytest.raises(ra.RustpotterError, match="gain normaliser is not available on a batch over a model bank"):
        sb.set_filters(gain)
    with pytest.raises(ra.RustpotterError, match="gain normaliser per model is not built"):
        sb.set_filters_bank(gain)
    # nothing above changed the batch: plain process, and the logits of a batch that was never refused anything
    det, n_det = sb.process(part)
    assert not n_det.any()
    fresh = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=2, model_bank=bank, stream_model=STREAM_MODEL)
    fresh.process_multi(part)
    assert np.array_equal(sb.logits().view(np.uint32), fresh.logits().view(np.uint32))
    # the band-pass alone is taken
    bp = ra.FiltersConfig()
    bp.band_pass.enabled = True
    sb2 = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=2, model_bank=bank, stream_model=STREAM_MODEL, filters=bp)
    sb2.process_multi(part)
    assert np.isfinite(sb2.logits()).all()
    # the calls of this feature on another kind of batch
    other = ra.StreamBatch(ctx, None, cfg, 1, max_chunks_per_call=2, wakewords=[{"model": models[0], "none_index": 0}], mfcc_size=K)
    with pytest.raises(ra.RustpotterError, match="not made by rp_stream_batch_new_model_bank"):
        other.set_models(0, np.zeros(1, np.int32))
    other.process_multi(part[:1])
    other.label_pitch = 2
    with pytest.raises(ra.RustpotterError, match="not made by rp_stream_batch_new_model_bank"):
        other.logits()
    # indices: outside the bank, an empty bank, every stream without a model, a bank of another context
    bad = STREAM_MODEL.copy()
    bad[7] = bank.W
    with pytest.raises(ra.RustpotterError, match="stream 7"):
        ra.StreamBatch(ctx, None, cfg, S, model_bank=bank, stream_model=bad)
    empty = ra.ModelBank(ctx, models=[])
    none = np.full(S, -1, np.int32)
    with pytest.raises(ra.RustpotterError, match="stream 0"):
        ra.StreamBatch(ctx, None, cfg, S, model_bank=empty, stream_model=np.zeros(S, np.int32))
    for b in (empty, bank):
        sbe = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=2, model_bank=b, stream_model=none)
        det, dww, dlab, n_det = sbe.process_multi(part)
        assert not n_det.any() and not det["frame"].any()
        lge = sbe.logits()
        assert lge.shape == (S, 6, b.label_pitch) and not lge.any()
    ctx2 = ra.BatchContext(device=0, host_pointers=True)
    with pytest.raises(ra.RustpotterError, match="another context"):
        ra.StreamBatch(ctx2, None, cfg, S, model_bank=bank, stream_model=STREAM_MODEL)


def test_device_pointers(ra, ctx, pcm, weights, one_chunk):
    """a device-pointer context: indices, audio, detections and logits on the device; an index outside the bank is treated as -1"""
    import torch
    dctx = ra.BatchContext(device=0, host_pointers=False)
    dbank = ra.ModelBank(dctx, models=[ra.Model(dctx, ws, bs) for ws, bs in weights], none_index=NONE_INDEX)
    idx = STREAM_MODEL.copy()
    idx[7] = dbank.W
    di = torch.from_numpy(idx).cuda()
    torch.cuda.synchronize()
    sb = ra.StreamBatch(dctx, None, config(ra), S, max_chunks_per_call=MAX_CHUNKS, model_bank=dbank, stream_model=di.data_ptr())
    max_det, itemsize = 12, np.dtype(ra.api.DET_DTYPE).itemsize
    x = torch.from_numpy(pcm).cuda()
    ddet = torch.zeros(S * max_det * itemsize, dtype=torch.uint8, device="cuda")
    dww = torch.zeros((S, max_det), dtype=torch.int32, device="cuda")
    dlab = torch.zeros((S, max_det), dtype=torch.int32, device="cuda")
    dn = torch.zeros(S, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    got, logits, c = [[] for _ in range(S)], [], 0
    while c < CHUNKS:
        n = min(10, CHUNKS - c)
        sb.process_multi_dev(x.data_ptr() + 4 * 480 * c, 3, n, pcm.shape[1], ddet.data_ptr(), dww.data_ptr(), dlab.data_ptr(), dn.data_ptr(), max_det)
        dl = torch.full((S, 3 * n, 3), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        sb.logits_dev(dl.data_ptr())
        dctx.synchronize()
        logits.append(dl.cpu().numpy())
        det = ddet.cpu().numpy().view(ra.api.DET_DTYPE).reshape(S, max_det)
        hn, hw, hl = dn.cpu().numpy(), dww.cpu().numpy(), dlab.cpu().numpy()
        for s in range(S):
            for i in range(hn[s]):
                d = det[s][i]
                got[s].append((int(d["frame"]), int(d["window"]), int(d["counter"]), bits1(d["score"]), bits1(d["avg_score"]), int(hw[s][i]), int(hl[s][i])))
        c += n
    lg = np.concatenate(logits, axis=1)
    assert not got[7] and not lg[7].any()
    keep = [s for s in range(S) if s != 7]
    assert [got[s] for s in keep] == [one_chunk[0][s] for s in keep]
    same_logits(lg[keep], one_chunk[1][keep], STREAM_MODEL[keep])


def test_resampled_input(ra, ctx, bank, models, pcm):
    """rp_stream_batch_set_input works as everywhere: 22.05 kHz input has 40 ms frames, four MFCC frames a chunk -- the cut into calls changes
    no bit, and the detections are those of the shared-model live batch with the stream's model"""
    cfg = config(ra)
    spc = ra.resampler_frame_lengths(22050)[0]
    chunks = 48000 // spc
    audio = np.ascontiguousarray(pcm[:, :chunks * spc])

    def run(sb, x, pieces, logits):
        assert sb.samples_per_chunk == spc and sb.frames_per_chunk == 4
        out, lgs, c, k = [[] for _ in range(x.shape[0])], [], 0, 0
        while c < chunks:
            n = min(pieces[k % len(pieces)], chunks - c)
            k += 1
            det, dww, dlab, n_det = sb.process_multi(np.ascontiguousarray(x[:, c * spc:(c + n) * spc]), max_det=8)
            for s in range(x.shape[0]):
                out[s] += [(int(d["frame"]), int(d["window"]), int(d["counter"]), bits1(d["score"]), bits1(d["avg_score"]), int(dlab[s][i]))
                           for i, d in enumerate(det[s][:n_det[s]])]
            if logits:
                lgs.append(sb.logits())
                assert lgs[-1].shape[1] == 4 * n
            c += n
        return out, (np.concatenate(lgs, axis=1) if logits else None)

    def batch(pieces):
        sb = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=7, sample_rate=22050, model_bank=bank, stream_model=STREAM_MODEL)
        return run(sb, audio, pieces, True)

    det, lg = batch((1,))
    det2, lg2 = batch((7, 2))
    assert det2 == det
    same_logits(lg2, lg, STREAM_MODEL)
    for s in (0, 1, 6):
        mi = STREAM_MODEL[s]
        sb = ra.StreamBatch(ctx, None, cfg, 1, max_chunks_per_call=7, sample_rate=22050, wakewords=[{"model": models[mi], "none_index": NONE_INDEX[mi]}], mfcc_size=K)
        want, _ = run(sb, audio[s:s + 1], (7, 2), False)
        assert want[0] == det[s], (s, want[0], det[s])
    print("22.05 kHz input: detections per stream", [len(d) for d in det])
