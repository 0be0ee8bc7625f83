"""Personal wakeword models: a model bank (rp_model_bank) and calls in which stream s is run by ITS model bank[stream_model[s]]
(rp_mlp_forward_windows_bank, rp_batch_detect_model_bank; mlp_windows_bank_kernel).  The yardstick is the shared-model path one stream at a
time: rp_mlp_forward_windows / rp_batch_detect_model with that stream's model.  A stream is cut into workgroups from its own window count,
so wherever the shared-model path takes mlp_windows_kernel (32 windows or more) the bank call must give the same BITS; a shorter stream is
one partial tile of the bank kernel against mlp_mfma_kernel on the other side: 2e-6 on scores.
Six models within the bank's limits; with 430 frames their window counts cover every edge of the cut: L 30 -> 401 windows (two workgroups,
7 + 6 tiles, the last partial), 75 -> 356 (two of 6 tiles), 195 -> 236 (two of 4), 256 -> 175 (one of 6); 226 frames are exactly 32 windows of
an L = 195 model, 220 frames 26 (the short-stream case), 190 frames none."""
import numpy as np
import pytest

from oracle import rp_oracle as orc
import rpw_py

pytestmark = pytest.mark.gpu
K = 16
# (model type, train_size L, hidden widths, labels); "none" is label 0 of models 1-5, model 6 has none
MODELS = [
    ("tiny", 30, (2,), ["none", "a"]),
    ("tiny", 195, (13,), ["none", "a"]),
    ("small", 75, (12, 6), ["none", "a", "b"]),
    ("small", 195, (32, 16), ["none", "a"]),
    ("tiny", 256, (17,), ["none", "a", "b"]),
    ("tiny", 195, (13,), ["a", "b"]),
]
NONE_INDEX = [0, 0, 0, 0, 0, -1]
# S = 13: every model at least twice, one stream without a model, shuffled
STREAM_MODEL = np.array([3, 0, 5, -1, 1, 4, 2, 0, 3, 5, 1, 2, 4], np.int32)
S = len(STREAM_MODEL)
WANT_KERNEL = "mlp_windows_kernel<bf16x3 splits>"
MODEL_SEED = 5
# detection: its own six models of the same shapes.  A detection ends when no window has passed for L / 2 frames, so on 3 s of steady noise
# a random model fires only if the threshold cuts THROUGH its scores: the last layer times 2 makes the scores move from window to window,
# and seed and threshold were chosen with oracle.rp_oracle.Detector.add_model on the CPU (rp_synth_pcm_batch's noise, min_scores 1, both
# avg_thresholds): 5 of the 12 streams with a model fire (1 or 2 detections each), 7 do not, label indices 0 (the model without a "none"
# label) and 1 occur, and no score lies within 2e-3 of the threshold.  With VADMode.Easy the oracle reports nothing on this noise: that
# case checks that the bank path gates as the shared-model path does.
DET_MODEL_SEED, DET_GAIN = 16, 2.0
DET_SEED = 0x5EED000000000001
DET_THRESHOLD = 0.7


def bank_weights(seed=MODEL_SEED, gain=1.0):
    """the six random models: [(ws, bs)], W_l [out][in] scaled by 1 / sqrt(in), biases 0.1 * N(0, 1); gain: a factor on the last layer's
    weights (the detection test: logits that move enough from window to window for a threshold to cut through them)"""
    rng = np.random.default_rng(seed)
    out = []
    for _, L, hidden, labels in MODELS:
        dims = [L * K] + list(hidden) + [len(labels)]
        ws = [(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32) for i in range(len(dims) - 1)]
        bs = [(rng.standard_normal(dims[i + 1]) * 0.1).astype(np.float32) for i in range(len(dims) - 1)]
        ws[-1] = (ws[-1] * np.float32(gain)).astype(np.float32)
        out.append((ws, bs))
    return out


def model_dict(i, ws, bs):
    """model i as tests/rpw_py.py and oracle.rp_oracle.Detector.add_model take it"""
    weights = {}
    for l, (w, b) in enumerate(zip(ws, bs)):
        weights["ln%d.weight" % (l + 1)] = w
        weights["ln%d.bias" % (l + 1)] = b
    return {"labels": MODELS[i][3], "train_size": MODELS[i][1], "mfcc_size": K, "m_type": MODELS[i][0], "weights": weights, "rms_level": float("nan")}


def synth_mfcc(rng, n_streams, nf):
    """rows with coefficient-dependent offsets about ten times their spread and a slow drift, as tests/test_gpu_mlp_range_and_windows.py"""
    off = rng.uniform(-30.0, 30.0, K).astype(np.float32)
    drift = np.linspace(0.0, 1.0, nf)[None, :, None] * rng.uniform(-6.0, 6.0, (n_streams, 1, K))
    return (rng.standard_normal((n_streams, nf, K)) * rng.uniform(0.5, 2.0, (n_streams, 1, 1)) + off + drift).astype(np.float32)


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


@pytest.fixture(scope="module")
def weights():
    return bank_weights()


@pytest.fixture(scope="module")
def models(ra, ctx, weights):
    return [ra.Model(ctx, ws, bs) for ws, bs in weights]


@pytest.fixture(scope="module")
def bank(ra, ctx, models):
    return ra.ModelBank(ctx, models=models, none_index=NONE_INDEX)


@pytest.fixture(scope="module")
def rows():
    """the MFCC rows of the calls, by frame count"""
    rng = np.random.default_rng(430)
    return {nf: synth_mfcc(rng, S, nf) for nf in (430, 226, 220, 190)}


@pytest.fixture(scope="module")
def yardstick(ctx, models, rows):
    """per frame count and stream: rp_mlp_forward_windows of that stream alone with its model (None without a model) and what ran"""
    out = {}
    for nf, mfcc in rows.items():
        per = []
        for s, mi in enumerate(STREAM_MODEL):
            if mi < 0:
                per.append((None, ""))
                continue
            lg = ctx.mlp_forward_windows(mfcc[s:s + 1], models[mi])[0]
            per.append((lg, ctx.last_mlp_kernel() if lg.shape[0] else ""))
        out[nf] = per
    return out


def n_win_of(nf, mi):
    return max(nf - MODELS[mi][1] + 1, 0) if mi >= 0 else 0


def check_rows(got, per, nf, idx=STREAM_MODEL, at_least=32):
    """row s of a bank call against the stream's own call, bit for bit where the stream has at_least windows; zeros behind windows and labels"""
    compared = 0
    for s, mi in enumerate(idx):
        nw, nl = n_win_of(nf, mi), (len(MODELS[mi][3]) if mi >= 0 else 0)
        assert not got[s, nw:].any() and not got[s, :, nl:].any(), s
        if nw >= at_least:
            want, ran = per[s]
            assert ran == WANT_KERNEL, (s, ran)
            assert want.shape == (nw, nl) and np.array_equal(got[s, :nw, :nl], want), (s, mi, nw)
            compared += 1
    return compared


@pytest.mark.parametrize("nf", [430, 226])
def test_forward_bit_for_bit(ctx, bank, rows, yardstick, nf):
    """every stream with 32 windows or more: the bits of rp_mlp_forward_windows over that stream alone with its model"""
    got = ctx.mlp_forward_windows_bank(rows[nf], bank, STREAM_MODEL)
    assert ctx.last_mlp_kernel() == "mlp_windows_bank_kernel<bf16x3 splits>"
    assert got.shape == (S, max(n_win_of(nf, mi) for mi in STREAM_MODEL), 3) and np.isfinite(got).all()
    compared = check_rows(got, yardstick[nf], nf)
    # 430 frames: every stream with a model; 226: exactly 32 windows for L = 195, none for L = 256
    assert compared == (12 if nf == 430 else 10)
    if nf == 226:
        assert [n_win_of(nf, mi) for mi in (1, 3, 5)] == [32, 32, 32] and n_win_of(nf, 4) == 0
    # a larger pitch only adds zero rows; bf16 is accepted and computes the same
    wide = ctx.mlp_forward_windows_bank(rows[nf], bank, STREAM_MODEL, win_pitch=got.shape[1] + 5)
    assert np.array_equal(wide[:, :got.shape[1]], got) and not wide[:, got.shape[1]:].any()
    assert np.array_equal(ctx.mlp_forward_windows_bank(rows[nf], bank, STREAM_MODEL, precision="bf16"), got)


def _scores(lg):
    """calc_inverse_similarity of label 1 against label 0 at score_ref 0.22 (wakeword_nn.rs:161-163: the reference is 10 score_ref)"""
    return np.array([orc.calc_inverse_similarity(float(r[1]), float(r[0]), 2.2) for r in lg], np.float64)


def test_short_streams(ctx, bank, weights, rows, yardstick):
    """26 windows: one partial tile of the bank kernel against mlp_mfma_kernel with each window's own mean on the shared-model path -- the
    two within 2e-6 on scores, both within 1e-5 of the oracle; 190 frames are shorter than the window: zero rows"""
    nf = 220
    got = ctx.mlp_forward_windows_bank(rows[nf], bank, STREAM_MODEL)
    check_rows(got, yardstick[nf], nf)   # L = 30 and 75 still have 32 windows or more: bits
    seen = 0
    for s, mi in enumerate(STREAM_MODEL):
        if mi < 0 or MODELS[mi][1] != 195:
            continue
        want, ran = yardstick[nf][s]
        assert want.shape[0] == 26 and ran.startswith("mlp_mfma_kernel<bf16x3 splits>"), ran
        a, b = _scores(got[s, :26]), _scores(want)
        print("stream %d model %d: bank against per-stream scores %.3g" % (s, mi, np.abs(a - b).max()))
        assert np.abs(a - b).max() <= 2e-6
        ws, bs = weights[mi]
        win = np.stack([orc.normalize(rows[nf][s, w:w + 195]).reshape(-1) for w in range(26)])
        ref = _scores(orc.mlp_forward(win, ws, bs))
        print("stream %d model %d: against the oracle %.3g / %.3g" % (s, mi, np.abs(a - ref).max(), np.abs(b - ref).max()))
        assert np.abs(a - ref).max() <= 1e-5 and np.abs(b - ref).max() <= 1e-5
        seen += 1
    assert seen == 6
    short = ctx.mlp_forward_windows_bank(rows[190], bank, STREAM_MODEL)
    for s, mi in enumerate(STREAM_MODEL):
        if mi >= 0 and MODELS[mi][1] >= 195:
            assert not short[s].any()
    check_rows(short, yardstick[190], 190)


def test_batch_invariance(ctx, bank, rows):
    """the same streams in another order, and a stream alone, give identical rows"""
    nf = 430
    got = ctx.mlp_forward_windows_bank(rows[nf], bank, STREAM_MODEL)
    perm = np.random.default_rng(1).permutation(S)
    again = ctx.mlp_forward_windows_bank(rows[nf][perm], bank, STREAM_MODEL[perm], win_pitch=got.shape[1])
    assert np.array_equal(again, got[perm])
    for s in (0, 1, 5, 6):
        nw = n_win_of(nf, STREAM_MODEL[s])
        one = ctx.mlp_forward_windows_bank(rows[nf][s:s + 1], bank, STREAM_MODEL[s:s + 1])
        assert one.shape[1] == nw and np.array_equal(one[0], got[s, :nw])


@pytest.fixture(scope="module")
def det_pcm(ctx):
    return ctx.synth_pcm(DET_SEED, 0, S, 480 * 100)


@pytest.fixture(scope="module")
def det_models(ra, ctx):
    return [ra.Model(ctx, ws, bs) for ws, bs in bank_weights(DET_MODEL_SEED, DET_GAIN)]


@pytest.mark.parametrize("avg_threshold,vad", [(0.0, None), (0.2, None), (0.0, "easy")])
def test_detection_equals_batch_detect_model_per_stream(ra, ctx, det_models, det_pcm, avg_threshold, vad):
    """rp_batch_detect_model_bank against one rp_batch_detect_model per stream with its model and none_index: the same detections, labels
    included, scores bit for bit"""
    det_bank = ra.ModelBank(ctx, models=det_models, none_index=NONE_INDEX)
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold, cfg.min_scores = avg_threshold, DET_THRESHOLD, 1
    if vad:
        cfg.vad_mode = ra.VADMode.Easy
    det, dlab, n_det = ctx.batch_detect_model_bank(det_pcm, det_bank, STREAM_MODEL, cfg)
    fired, labels = 0, set()
    for s, mi in enumerate(STREAM_MODEL):
        if mi < 0:
            assert n_det[s] == 0
            continue
        want, wlab, wn = ctx.batch_detect_model(det_pcm[s:s + 1], det_models[mi], K, NONE_INDEX[mi], cfg)
        assert ctx.last_mlp_kernel() == WANT_KERNEL
        assert n_det[s] == wn[0], (s, mi, n_det[s], wn[0])
        fired += wn[0] > 0
        for j in range(min(int(wn[0]), det.shape[1])):
            a, b = det[s][j], want[0][j]
            assert a["stream"] == s
            assert all(a[f] == b[f] for f in ("frame", "window", "counter")) and dlab[s][j] == wlab[0][j], (s, j, a, b)
            assert a["score"].tobytes() == b["score"].tobytes() and a["avg_score"].tobytes() == b["avg_score"].tobytes(), (s, j, a, b)
            labels.add(int(wlab[0][j]))
    print("avg_threshold %g vad %s: %d of 12 streams fire, labels %s" % (avg_threshold, vad, fired, sorted(labels)))
    # the yardstick's output is no empty comparison
    if vad is None:
        assert 3 * fired >= 12 and fired < 12 and len(labels) >= 2, (fired, labels)
    else:
        assert fired == 0   # as the oracle: the VAD hears no voice in steady noise -- and the bank path must gate like the yardstick


def test_indices(ra, ctx, bank, rows, det_pcm):
    """-1: a zero row and no detection; W under host pointers: an error that names the stream, nothing written; on a device-pointer context
    the kernels treat it as -1"""
    import torch
    nf = 430
    idx = STREAM_MODEL.copy()
    got = ctx.mlp_forward_windows_bank(rows[nf], bank, idx)
    assert not got[3].any()
    idx[7] = bank.W
    out = np.full((S, got.shape[1], 3), 7.0, np.float32)
    L = ra.load_library()
    assert L.rp_mlp_forward_windows_bank(ctx._h, bank._h, idx.ctypes.data, rows[nf].ctypes.data, S, nf, 0, out.ctypes.data, got.shape[1]) < 0
    assert "stream 7" in L.rp_last_error().decode() and (out == 7.0).all()
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.threshold, cfg.min_scores = 0.0, DET_THRESHOLD, 1
    with pytest.raises(ra.RustpotterError, match="stream 7"):
        ctx.batch_detect_model_bank(det_pcm, bank, idx, cfg)
    # device pointers: a bank of that context
    dctx = ra.BatchContext(device=0, host_pointers=False)
    dbank = ra.ModelBank(dctx, models=[ra.Model(dctx, ws, bs) for ws, bs in bank_weights()], none_index=NONE_INDEX)
    pitch = nf - 30 + 1   # the largest window count any model of the bank has
    x, di = torch.from_numpy(rows[nf]).cuda(), torch.from_numpy(idx).cuda()
    dout = torch.full((S, pitch, 3), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dctx.mlp_forward_windows_bank_dev(dbank, di.data_ptr(), x.data_ptr(), S, nf, "f32", dout.data_ptr(), pitch)
    with pytest.raises(ra.RustpotterError, match="win_pitch"):
        dctx.mlp_forward_windows_bank_dev(dbank, di.data_ptr(), x.data_ptr(), S, nf, "f32", dout.data_ptr(), pitch - 1)
    dctx.synchronize()
    dgot = dout.cpu().numpy()
    assert not dgot[7].any()   # index W: no model
    keep = np.arange(S) != 7
    assert np.array_equal(dgot[keep][:, :got.shape[1]], got[keep]) and not dgot[:, got.shape[1]:].any()


def test_empty_bank_pitch_and_precisions(ra, ctx, bank, rows, det_pcm):
    nf = 430
    empty = ra.ModelBank(ctx, models=[])
    assert empty.W == 0 and empty.max_train_size == 0 and empty.label_pitch == 0
    none = np.full(S, -1, np.int32)
    assert ctx.mlp_forward_windows_bank(rows[nf], empty, none).shape == (S, 0, 0)
    cfg = ra.DetectorConfig()
    det, dlab, n_det = ctx.batch_detect_model_bank(det_pcm, empty, none, cfg)
    assert not n_det.any() and not det["frame"].any() and not dlab.any()
    with pytest.raises(ra.RustpotterError, match="stream 0"):
        ctx.mlp_forward_windows_bank(rows[nf], empty, np.zeros(S, np.int32))
    # win_pitch one below the largest window count of the call
    with pytest.raises(ra.RustpotterError, match="win_pitch"):
        ctx.mlp_forward_windows_bank(rows[nf], bank, STREAM_MODEL, win_pitch=400)
    for prec in ("f32_fast", "f32_strict"):
        with pytest.raises(ra.RustpotterError, match="RP_MLP_F32_FAST and RP_MLP_F32_STRICT"):
            ctx.mlp_forward_windows_bank(rows[nf], bank, STREAM_MODEL, precision=prec)
        with pytest.raises(ra.RustpotterError, match="RP_MLP_F32_FAST and RP_MLP_F32_STRICT"):
            ctx.batch_detect_model_bank(det_pcm, bank, STREAM_MODEL, cfg, precision=prec)


def _random_model(ra, ctx, rng, dims):
    ws = [(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32) for i in range(len(dims) - 1)]
    bs = [(rng.standard_normal(dims[i + 1]) * 0.1).astype(np.float32) for i in range(len(dims) - 1)]
    return ra.Model(ctx, ws, bs)


def test_limits_are_named(ra, ctx):
    rng = np.random.default_rng(9)
    ok = _random_model(ra, ctx, rng, (40 * 16, 8, 2))
    with pytest.raises(ra.RustpotterError, match=r"model 1: layer 1 is 65 wide.*at most 32"):      # a Medium model
        ra.ModelBank(ctx, models=[ok, _random_model(ra, ctx, rng, (195 * 16, 65, 32, 2))])
    with pytest.raises(ra.RustpotterError, match=r"mfcc_size 13 is not built.*mfcc_size 16"):
        ra.ModelBank(ctx, models=[_random_model(ra, ctx, rng, (40 * 13, 8, 2))], mfcc_size=13)
    with pytest.raises(ra.RustpotterError, match=r"model 0: a window of 257 frames.*at most 256"):
        ra.ModelBank(ctx, models=[_random_model(ra, ctx, rng, (257 * 16, 8, 2))])
    with pytest.raises(ra.RustpotterError, match=r"model 0: layer 2 is 33 wide.*at most 32"):
        ra.ModelBank(ctx, models=[_random_model(ra, ctx, rng, (40 * 16, 8, 33, 2))])
    with pytest.raises(ra.RustpotterError, match="none_index out of range"):
        ra.ModelBank(ctx, models=[ok], none_index=[2])


def test_bank_from_rpw_and_freed_handles(ra, ctx, bank, weights, rows):
    """.rpw bytes give the bits of the bank built from handles (labels -> none_index); files of two mfcc sizes are refused; the bank holds
    copies: freeing the rp_model handles changes nothing"""
    nf = 430
    got = ctx.mlp_forward_windows_bank(rows[nf], bank, STREAM_MODEL)
    files = []
    for i, (ws, bs) in enumerate(weights):
        m = model_dict(i, ws, bs)
        files.append(rpw_py.dump_rpw_model(m["labels"], m["train_size"], K, m["m_type"], m["weights"]))
    fbank = ra.ModelBank(ctx, rpw=files)
    assert fbank.W == 6 and fbank.train_sizes == [m[1] for m in MODELS] and fbank.labels == [len(m[3]) for m in MODELS]
    assert np.array_equal(ctx.mlp_forward_windows_bank(rows[nf], fbank, STREAM_MODEL), got)
    rng = np.random.default_rng(2)
    w13 = [(rng.standard_normal((4, 20 * 13)) * 0.1).astype(np.float32), (rng.standard_normal((2, 4)) * 0.1).astype(np.float32)]
    other = rpw_py.dump_rpw_model(["none", "a"], 20, 13, "tiny", {"ln1.weight": w13[0], "ln1.bias": np.zeros(4, np.float32),
                                                                    "ln2.weight": w13[1], "ln2.bias": np.zeros(2, np.float32)})
    with pytest.raises(ra.RustpotterError, match="wakeword 1: Usage of wakewords with different mfcc size"):
        ra.ModelBank(ctx, rpw=[files[0], other])
    temp = [ra.Model(ctx, ws, bs) for ws, bs in weights]
    tbank = ra.ModelBank(ctx, models=temp, none_index=NONE_INDEX)
    del temp[:]
    import gc
    gc.collect()
    scratch = [_random_model(ra, ctx, rng, (195 * 16, 32, 16, 2)) for _ in range(6)]   # what the allocator hands out next
    assert np.array_equal(ctx.mlp_forward_windows_bank(rows[nf], tbank, STREAM_MODEL), got)
    assert len(scratch) == 6
