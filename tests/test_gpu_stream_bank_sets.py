"""Wakeword sets on live streams (rp_stream_batch_new_bank_sets / _set_wakeword_sets / _slot_scores; dtw_set_stream_kernel,
scan_set_stream_kernel): stream s holds up to eight wakewords of a bank and is fed chunk by chunk.  Checked bit for bit against the
whole-recording call over the concatenation (rp_batch_detect_bank_sets), against the bank batch where a set holds one wakeword, and against the
CPU oracle's detector with several add_ref where a stream is re-targeted.  ctx.dtw_ref_pairs() must not move (see test_gpu_bank_sets.py)."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_bank_sets as wb
import test_gpu_stream_bank as sbk

pytestmark = pytest.mark.gpu

GOLDEN_RPW = sbk.GOLDEN_RPW
SETS_STREAM = "dtw_set_stream_kernel"
bits, read, feed = sbk.bits, sbk.read, sbk.feed
ra, ctx, golden = wb.ra, wb.ctx, wb.golden   # the fixtures of the whole-recording tests (module-scoped: made once more for this module)


@pytest.fixture(scope="module")
def streams():
    """seven streams of about 5.5 s and their sets: every pair of the golden bank, the triple, a hole, a duplicate, nobody"""
    rng = np.random.default_rng(61)
    names = ["alexa.wav", "oye_casa_g_1.wav", "oye_casa_real_1.wav", "oye_casa_g_1.wav", "oye_casa_real_1.wav", "oye_casa_g_2.wav", "alexa.wav"]
    sets = [[0, 1, -1], [1, 2, 0], [0, -1, 2], [-1, 1, -1], [2, 2, 1], [-1, -1, -1], [1, 2, -1]]
    return wb.stack([wb.padded(rng, wb.recording(n)) for n in names]), sets


@pytest.fixture(scope="module")
def whole(ra, ctx, golden, streams):
    bank, _ = golden
    pcm, sets = streams
    before = ctx.dtw_ref_pairs()
    ref, _, _ = wb.detect_sets(ctx, bank, pcm, sets, ra.DetectorConfig())
    assert ctx.dtw_ref_pairs() == before
    assert sum(len(v) for v in ref) >= 5 and not ref[5]
    return ref


def live_tuples(live):
    """feed()'s records as detect_sets()'s: (frame, window, counter, score bits, avg bits, bank index); the label must be -1"""
    assert all(d[6] == -1 for v in live for d in v)
    return [[d[:6] for d in v] for v in live]


@pytest.mark.parametrize("pieces", [(1,), (8,), (3, 1, 2)])
def test_live_equals_whole(ra, ctx, golden, streams, whole, pieces):
    """1. Fed in pieces, every stream reports the detections of rp_batch_detect_bank_sets over the concatenation: n_det, frame, window,
    counter, score and avg bits and the winner's bank index."""
    bank, _ = golden
    pcm, sets = streams
    before, arith = ctx.dtw_ref_pairs(), ctx.get_arithmetic()
    ctx.dtw_kernels()
    sb = ra.StreamBatch(ctx, None, ra.DetectorConfig(), len(sets), max_chunks_per_call=8, bank=bank, stream_wakewords=sets)
    live, _ = feed(sb, pcm, pieces)
    assert SETS_STREAM in ctx.dtw_kernels() and ctx.get_arithmetic() == arith
    assert ctx.dtw_ref_pairs() == before
    assert live_tuples(live) == whole, (live, whole)
    # rp_stream_batch_process without agg works too and reports the same
    sb2 = ra.StreamBatch(ctx, None, ra.DetectorConfig(), len(sets), max_chunks_per_call=8, bank=bank, stream_wakewords=sets)
    det, n_det = sb2.process(pcm[:, :480 * 8])
    assert not n_det.any()


def feed_slots(sb, pcm, per_call, before_chunk=None):
    """feed() that also collects rp_stream_batch_slot_scores of every call -> detections, agg, avg [S][set_size][frames]"""
    spc = sb.samples_per_chunk
    total = pcm.shape[1] // spc
    out, aggs, avgs = [[] for _ in range(pcm.shape[0])], [], []
    for c in range(0, total, per_call):
        n = min(per_call, total - c)
        if before_chunk is not None:
            before_chunk(c)
        det, dww, dlab, n_det = sb.process_multi(np.ascontiguousarray(pcm[:, c * spc:(c + n) * spc]), max_det=8)
        for s in range(pcm.shape[0]):
            for i in range(n_det[s]):
                d = det[s][i]
                out[s].append((int(d["frame"]), int(d["window"]), int(d["counter"]), sbk.bits1(d["score"]), sbk.bits1(d["avg_score"]), int(dww[s][i])))
        a, v = sb.slot_scores()
        assert a.shape == (pcm.shape[0], sb.set_size, n * sb.frames_per_chunk)
        aggs.append(a)
        avgs.append(v)
    return out, np.concatenate(aggs, axis=2), np.concatenate(avgs, axis=2)


def same_slot_scores(bank, sets, live, ref, first_frame=0, fpc=3):
    """the live slot score at frame f >= Lmax(s) - 1 is the whole call's slot row at f - Lmax(s) + 1 (column j of the live rows is frame j - fpc)"""
    n = 0
    for s, row in enumerate(sets):
        L = wb.lmax_of(bank, row)
        if not L:
            assert not live[s].any()
            continue
        f = np.arange(max(L - 1, first_frame), live.shape[2] - fpc)
        assert len(f) > 0
        for j, w in enumerate(row):
            if w < 0:
                assert not live[s, j].any(), (s, j)
                continue
            a, b = bits(live[s, j][f + fpc]), bits(ref[s, j][f - L + 1])
            assert np.array_equal(a, b), (s, j, "differs in %d of %d windows" % (int(np.sum(a != b)), len(f)))
            n += len(f)
    return n


def test_slot_scores_equal_the_whole_call(ra, streams):
    """2. On a RP_CTX_FULL_SCORES context the slot scores of every call are the whole call's slot rows, agg and avg; before the first call
    rp_stream_batch_slot_scores fails."""
    full = ra.BatchContext(device=0, host_pointers=True, full_scores=True)
    bank = ra.WakewordBank(full, rpw=[read(n) for n in GOLDEN_RPW])
    pcm, sets = streams
    cfg = ra.DetectorConfig()
    ref, r_agg, r_avg = wb.detect_sets(full, bank, pcm, sets, cfg, want_agg=True)
    sb = ra.StreamBatch(full, None, cfg, len(sets), max_chunks_per_call=4, bank=bank, stream_wakewords=sets)
    with pytest.raises(ra.RustpotterError, match="have not received audio yet"):
        sb.slot_scores()
    live, agg, avg = feed_slots(sb, pcm, 4)
    assert full.dtw_ref_pairs() == 0
    assert live == ref
    n = same_slot_scores(bank, sets, agg, r_agg) + same_slot_scores(bank, sets, avg, r_avg)
    print("%d slot scores bit-equal" % n)


def test_retargeting(ra, ctx, golden, streams):
    """3. rp_stream_batch_set_wakeword_sets in mid-stream: to another set, to all -1 and back.  A re-targeted stream reports, from then on,
    what a stream that always held the new set and was reset at that chunk reports -- and what a fresh oracle detector fed from that chunk
    on reports; the other streams never notice; all -1 reports nothing."""
    bank, dicts = golden
    pcm, _ = streams
    x = pcm[[1, 1, 2, 1, 3]]
    cfg = ra.DetectorConfig()
    c0 = 10   # before the utterances: the window refills in time
    before = ctx.dtw_ref_pairs()
    A = ra.StreamBatch(ctx, None, cfg, 5, bank=bank, stream_wakewords=[[0, 1], [1, 0], [0, 2], [0, 1], [1, -1]])
    B = ra.StreamBatch(ctx, None, cfg, 5, bank=bank, stream_wakewords=[[2, -1], [-1, -1], [0, 2], [0, 1], [1, -1]])

    def act_a(c):
        if c == c0:
            A.reset(0)
            A.reset(1)

    def act_b(c):
        if c == 4:
            B.set_wakeword_sets(3, [[-1, -1]])          # nobody ...
        if c == 6:
            B.set_wakeword_sets(3, [[0, 1]])            # ... and back, long before the utterance
        if c == c0:
            B.set_wakeword_sets(0, [[0, 1], [1, 0]])    # another set; -1 -> a set
            B.set_wakeword_sets(4, [[-1, -1]])
    live_a, _ = feed(A, x, (1,), before_chunk=act_a)
    live_b, _ = feed(B, x, (1,), before_chunk=act_b)
    assert ctx.dtw_ref_pairs() == before
    frame0 = 3 * c0 - 3
    for s in (0, 1):
        from_c = [d for d in live_a[s] if d[0] >= frame0]
        assert from_c and [d for d in live_b[s] if d[0] >= frame0] == from_c, (s, live_a[s], live_b[s])
        # the oracle counterpart: a fresh detector from chunk c0 on (its chunk k is the batch's chunk c0 + k)
        row = [[0, 1], [1, 0]][s]
        want = [(c0 + k, r) for k, r in wb.oracle_sets(dicts, row, x[s][480 * c0:], cfg)]
        wb.same_as_oracle(dicts, bank, row, [d[:6] for d in from_c], want)
    assert not [d for d in live_b[1] if d[0] < frame0], "a stream without wakewords reports nothing"
    assert live_b[2] == live_a[2] and live_a[2], "the other streams are untouched"
    assert live_b[3] == live_a[3] and live_a[3], "re-targeted to nobody and back before the utterance: reset twice, the same detections"
    assert live_a[4] and not [d for d in live_b[4] if d[0] >= frame0], "a set -> all -1 reports nothing afterwards"


def test_a_changing_bank(ra, streams):
    """4. rp_wakeword_bank_put under the batch replaces wakeword 1 by a longer one within the reserved length: from the next call the streams
    that hold it score with the new Lmax(s) (their slot scores are those of the whole call over the NEW bank), the others keep their bits."""
    import rpw_py, os
    full = ra.BatchContext(device=0, host_pointers=True, full_scores=True)
    bank = ra.WakewordBank(full, rpw=[read(n) for n in GOLDEN_RPW])
    bank.reserve(max_len=200)
    d = rpw_py.load_rpw(os.path.join(sbk.G, "oye_casa_real.rpw"))
    longer = [np.concatenate([t, t[:190 - len(t)]]).astype(np.float32) for t in list(d["samples_features"].values())[:2]]
    assert all(len(t) == 190 for t in longer)
    pcm, _ = streams
    x = pcm[[1, 2, 0]]
    sets = [[1, 0], [0, 1], [0, 2]]     # Lmax 126, 126, 168 -> 190, 190, 168
    cfg = ra.DetectorConfig()
    quiet_run = ra.StreamBatch(full, None, cfg, 3, max_chunks_per_call=4, bank=bank, stream_wakewords=sets)
    _, agg0, _ = feed_slots(quiet_run, x, 4)
    quiet_run.close()
    sb = ra.StreamBatch(full, None, cfg, 3, max_chunks_per_call=4, bank=bank, stream_wakewords=sets)
    c0 = 80
    _, agg1, _ = feed_slots(sb, x, 4, before_chunk=lambda c: bank.put(1, [(longer, None, None, None)]) if c == c0 else None)
    assert bank.max_lens == [126, 190, 168]
    assert np.array_equal(bits(agg1[2]), bits(agg0[2])), "a stream that does not hold the wakeword keeps its bits"
    col = 3 + 3 * c0 - 3   # the first column of the call that followed the put
    assert np.array_equal(bits(agg1[:, :, :col]), bits(agg0[:, :, :col]))
    _, r_agg, _ = wb.detect_sets(full, bank, x, sets, cfg, want_agg=True)
    n = same_slot_scores(bank, sets, agg1, r_agg, first_frame=3 * c0 - 3)
    assert n > 0 and full.dtw_ref_pairs() == 0
    print("%d slot scores after the put bit-equal to the whole call over the new bank" % n)


@pytest.mark.parametrize("case", ["48k", "band_pass"])
def test_one_wakeword_sets_equal_the_bank_batch(ra, ctx, golden, streams, case):
    """5. At 48 kHz through rp_stream_batch_set_input and with the band-pass filter alone: sets that hold one wakeword (in either slot) against
    the bank batch of those wakewords, and sets of two wakewords against the shared live batch of the two under RP_ARITH_STRICT_F32 -- the
    same detections, bit for bit."""
    bank, dicts = golden
    pcm16, _ = streams
    idx = [1, 2, 0]
    sets = [[1, -1], [-1, 2], [0, 0]]
    rate = 48000 if case == "48k" else 16000
    kw = {}
    if case == "band_pass":
        f = ra.FiltersConfig()
        f.band_pass.enabled, f.band_pass.low_cutoff, f.band_pass.high_cutoff = True, 80.0, 2000.0
        kw = dict(filters=f)
    cfg = ra.DetectorConfig()
    a = ra.StreamBatch(ctx, None, cfg, 3, max_chunks_per_call=4, sample_rate=rate, bank=bank, stream_wakewords=sets, **kw)
    b = ra.StreamBatch(ctx, None, cfg, 3, max_chunks_per_call=4, sample_rate=rate, bank=bank, stream_wakeword=idx, **kw)
    spc = a.samples_per_chunk
    x = [pcm16[s] if rate == 16000 else sbk.resampled(pcm16[s], rate) for s in (1, 2, 0)]
    n = spc * (min(len(v) for v in x) // spc)
    x = np.stack([v[:n] for v in x])
    before = ctx.dtw_ref_pairs()
    live_a, _ = feed(a, x, (4, 1))
    live_b, _ = feed(b, x, (4, 1))
    assert ctx.dtw_ref_pairs() == before
    assert live_a == live_b and sum(len(v) for v in live_a) >= 2, (live_a, live_b)
    # ... and sets of two different wakewords against the shared live batch that holds the two (rp_stream_batch_new_multi, strict f32),
    # behind the same resampler / filter: Lmax over the slots and the per-frame proposal over them
    pair = [0, 1]
    c = ra.StreamBatch(ctx, None, cfg, 3, max_chunks_per_call=4, sample_rate=rate, bank=bank, stream_wakewords=[pair] * 3, **kw)
    specs = [dict(templates=ra.Templates(ctx, list(dicts[w]["samples_features"].values()), dicts[w]["avg_features"]),
                  threshold=dicts[w]["threshold"], avg_threshold=dicts[w]["avg_threshold"]) for w in pair]
    m = ra.StreamBatch(ctx, None, cfg, 3, max_chunks_per_call=4, sample_rate=rate, wakewords=specs, mfcc_size=5, **kw)
    live_c, _ = feed(c, x, (4, 1))
    with ctx.arithmetic("strict_f32"):
        live_m, _ = feed(m, x, (4, 1))
    assert ctx.dtw_ref_pairs() == before
    assert live_c == [[d[:5] + (pair[d[5]], d[6]) for d in v] for v in live_m], (live_c, live_m)
    assert {d[5] for v in live_c for d in v} == {0, 1}, "both wakewords of the set win somewhere"


def test_device_pointer_context(ra, streams, whole):
    """6. A context without RP_CTX_HOST_POINTERS: sets, audio and outputs on the device; an index outside the bank is treated as -1."""
    import torch
    pcm, sets = streams
    S, max_det = len(sets), 4
    dctx = ra.BatchContext(device=0, host_pointers=False)
    bank = ra.WakewordBank(dctx, rpw=[read(n) for n in GOLDEN_RPW])
    bad = [list(r) for r in sets]
    bad[0][2], bad[3][0], bad[5][1] = 3, -9, 77      # empty slots of the plan, now outside the bank
    d_sets = torch.tensor(bad, dtype=torch.int32, device="cuda")
    sb = ra.StreamBatch(dctx, None, ra.DetectorConfig(), S, max_chunks_per_call=8, bank=bank, stream_wakewords=int(d_sets.data_ptr()), set_size=3)
    d_pcm = torch.from_numpy(pcm).cuda()
    d_det = torch.zeros(S * max_det * 24, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(S, dtype=torch.int32, device="cuda")
    d_ww = torch.zeros(S * max_det, dtype=torch.int32, device="cuda")
    d_lab = torch.zeros(S * max_det, dtype=torch.int32, device="cuda")
    d_slots = torch.zeros(S * 3 * 24, dtype=torch.float32, device="cuda")
    got = [[] for _ in range(S)]
    total = pcm.shape[1] // 480
    for c in range(0, total, 8):
        n = min(8, total - c)
        part = d_pcm[:, c * 480:(c + n) * 480].contiguous()
        sb.process_multi_dev(part.data_ptr(), 3, n, n * 480, d_det.data_ptr(), d_ww.data_ptr(), d_lab.data_ptr(), d_n.data_ptr(), max_det)
        sb.slot_scores_dev(d_slots.data_ptr(), None)
        dctx.synchronize()
        det = np.frombuffer(d_det.cpu().numpy().tobytes(), dtype=ra.api.DET_DTYPE).reshape(S, max_det)
        nd, ww, lab = d_n.cpu().numpy(), d_ww.cpu().numpy().reshape(S, max_det), d_lab.cpu().numpy().reshape(S, max_det)
        for s in range(S):
            for i in range(nd[s]):
                d = det[s][i]
                got[s].append((int(d["frame"]), int(d["window"]), int(d["counter"]), sbk.bits1(d["score"]), sbk.bits1(d["avg_score"]), int(ww[s][i])))
                assert lab[s][i] == -1
    assert dctx.dtw_ref_pairs() == 0
    assert got == whole
    d_two = torch.tensor([[1, 9, -1], [2, 2, 2]], dtype=torch.int32, device="cuda")
    sb.set_wakeword_sets(0, int(d_two.data_ptr()), n=2)
    dctx.synchronize()


def test_refusals(ra, ctx, golden):
    """7. The refusals of the batch calls, each with its message; what must keep working on a sets batch does."""
    bank, dicts = golden
    cfg = ra.DetectorConfig()
    L = ra.load_library()
    c = cfg._c()
    h = C.c_void_p()
    idx = np.array([[0, 1], [2, -1]], np.int32)
    new = L.rp_stream_batch_new_bank_sets
    assert new(ctx._h, None, idx.ctypes.data, 2, C.byref(c), 2, 1, C.byref(h)) == -1 and b"null handle" in L.rp_last_error()
    assert new(ctx._h, bank._h, None, 2, C.byref(c), 2, 1, C.byref(h)) == -1 and b"null argument" in L.rp_last_error()
    assert new(ctx._h, bank._h, idx.ctypes.data, 2, None, 2, 1, C.byref(h)) == -1 and b"null argument" in L.rp_last_error()
    assert new(ctx._h, bank._h, idx.ctypes.data, 2, C.byref(c), 0, 1, C.byref(h)) == -1 and b"rp_stream_batch_new_bank_sets: S and max_chunks_per_call must be >= 1" in L.rp_last_error()
    for n in (0, 9):
        assert new(ctx._h, bank._h, idx.ctypes.data, n, C.byref(c), 2, 1, C.byref(h)) == -1 and b"set_size %d is outside 1 .. 8" % n in L.rp_last_error()
    for bad in (3, -2):
        with pytest.raises(ra.RustpotterError, match=r"^stream 1, slot 2: wakeword index %d is outside the bank \(-1 .. 2\)" % bad):
            ra.StreamBatch(ctx, None, cfg, 2, bank=bank, stream_wakewords=[[0, 1, 2], [0, 1, bad]])
    other = ra.BatchContext(device=0, host_pointers=True)
    with pytest.raises(ra.RustpotterError, match="the bank belongs to another context"):
        ra.StreamBatch(other, None, cfg, 2, bank=bank, stream_wakewords=idx)
    sb = ra.StreamBatch(ctx, None, cfg, 2, max_chunks_per_call=2, bank=bank, stream_wakewords=idx)
    with pytest.raises(ra.RustpotterError, match="a batch of several wakewords has no single aggregate per window"):
        sb.process(np.zeros((2, 480), np.float32), want_agg=True)
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_wakewords: the batch holds wakeword sets"):
        sb.set_wakewords(0, [1])
    f = ra.FiltersConfig()
    f.gain_normalizer.enabled = True
    with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_filters_bank: the gain normaliser is not available on a batch over wakeword sets"):
        sb.set_filters_bank(f)
    with pytest.raises(ra.RustpotterError, match="gain normaliser is not available"):
        sb.set_filters(f, 0.05)
    with pytest.raises(ra.RustpotterError, match=r"rp_stream_batch_set_wakeword_sets: streams 1 .. 1 \+ 2 reach past the batch's 2 streams"):
        sb.set_wakeword_sets(1, [[0, 1], [1, 2]])
    with pytest.raises(ra.RustpotterError, match=r"^stream 1, slot 0: wakeword index 5 is outside the bank"):
        sb.set_wakeword_sets(0, [[1, 2], [5, 0]])
    assert L.rp_stream_batch_set_wakeword_sets(sb._h, 0, 1, None) == -1 and b"null argument" in L.rp_last_error()
    assert L.rp_stream_batch_slot_scores(None, None, None) == -1 and b"null handle" in L.rp_last_error()
    sb.set_wakeword_sets(2, np.zeros((0, 2), np.int32))   # an empty range at the end is fine
    sb.reset(0)
    det, dww, dlab, n_det = sb.process_multi(np.zeros((2, 2 * 480), np.float32))   # the refusals above left the batch usable
    assert not n_det.any()
    plain = ra.StreamBatch(ctx, None, cfg, 2, bank=bank, stream_wakeword=[0, 1])
    tm = ra.Templates(ctx, list(dicts[1]["samples_features"].values()), dicts[1]["avg_features"])
    shared = ra.StreamBatch(ctx, tm, cfg, 2)
    for b in (plain, shared):
        with pytest.raises(ra.RustpotterError, match="rp_stream_batch_set_wakeword_sets: the batch was not made by rp_stream_batch_new_bank_sets"):
            b.set_wakeword_sets(0, [[0, 1]])
        b.process_multi(np.zeros((2, 480), np.float32))
        assert L.rp_stream_batch_slot_scores(b._h, None, None) == -1 and b"was not made by rp_stream_batch_new_bank_sets" in L.rp_last_error()
    # an empty bank, rows of all -1, band_size 0: calls succeed, zero slot scores, no detection
    rng = np.random.default_rng(3)
    noise = (0.1 * rng.standard_normal((2, 480 * 40))).astype(np.float32)
    empty = ra.WakewordBank(ctx, wakewords=[])
    zero = ra.DetectorConfig()
    zero.band_size = 0
    for bk, cf, ix in ((empty, cfg, [[-1, -1], [-1, -1]]), (bank, cfg, [[-1, -1], [-1, -1]]), (bank, zero, [[0, 1], [2, -1]])):
        sb = ra.StreamBatch(ctx, None, cf, 2, max_chunks_per_call=4, bank=bk, stream_wakewords=ix)
        live, agg, avg = feed_slots(sb, noise, 4)
        assert not any(live) and not agg.any() and not avg.any()
