"""Model sets over whole recordings: several personal wakeword models per stream over a model bank (rp_mlp_forward_windows_bank_sets,
rp_batch_detect_model_bank_sets; window_means_model_set_kernel, mlp_windows_model_set_kernel, nn_score_model_set_kernel,
scan_model_set_kernel).  Stream s is a Rustpotter with add_wakeword(model) per live slot of its row: one window of Lmax(s) frames, every
slot scoring the oldest L_j frames of it, the best passing score winning, the first slot of equals.
Yardsticks: the logits of row (s, j) are those of rp_mlp_forward_windows_bank over the first n_frames - (Lmax(s) - L_j) frames of the stream
with that model -- the same kernel body with the same cut, so BIT FOR BIT at every window count -- and, from 32 windows on, those of
rp_mlp_forward_windows.  The detections are those of a host fold of the call's own logits -- events exactly, scores within 1e-6 (host exp against expf) -- (tests/model_set_cases.py: fold_ref
through tests/nn_decide_ref.py and tests/scan_ref.py).  Bank, rows and audio: tests/model_set_cases.py.
Frame counts of the forward tests: 300 (several workgroups for the short windows), 220 (26 windows for the rows that hold a 195-frame
model: fewer than 32), 195 (exactly one), 120 (shorter than 195 but longer than 30, 47 and 96: every slot of such a row is zero)."""
import numpy as np
import pytest

import model_set_cases as M
import nn_decide_ref as R

pytestmark = pytest.mark.gpu
NFS = (300, 220, 195, 120)
WANT_KERNEL = "mlp_windows_kernel<bf16x3 splits>"
# (threshold, avg_threshold, vad, eager, min_scores): VAD off and on, eager off and on, avg_threshold 0 and not
CONFIGS = [(M.THRESHOLD, 0.0, None, False, 1), (M.THRESHOLD, M.AVG_THRESHOLD, None, True, 2), (M.THRESHOLD, 0.0, "easy", False, 1),
           (M.THRESHOLD, M.AVG_THRESHOLD, "easy", True, 2)]


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


@pytest.fixture(scope="module")
def models(ra, ctx):
    return [ra.Model(ctx, ws, bs) for ws, bs in M.bank_weights()]


@pytest.fixture(scope="module")
def bank(ra, ctx, models):
    return ra.ModelBank(ctx, models=models, none_index=M.NONE_INDEX)


@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(300)
    return {nf: M.synth_mfcc(rng, M.S, nf) for nf in NFS}


@pytest.fixture(scope="module")
def set_logits(ctx, bank, rows):
    """the sets call per frame count, computed once"""
    out = {}
    for nf in NFS:
        out[nf] = ctx.mlp_forward_windows_bank_sets(rows[nf], bank, M.SETS)
        assert ctx.last_mlp_kernel() == "mlp_windows_model_set_kernel<bf16x3 splits>"
    return out


def config(ra, threshold, avg_threshold, vad, eager, min_scores):
    cfg = ra.DetectorConfig()
    cfg.threshold, cfg.avg_threshold, cfg.eager, cfg.min_scores = threshold, avg_threshold, eager, min_scores
    if vad:
        cfg.vad_mode = ra.VADMode.Easy
    return cfg


@pytest.mark.parametrize("nf", NFS)
def test_slot_rows_bit_for_bit(ctx, bank, models, rows, set_logits, nf):
    """row (s, j) against rp_mlp_forward_windows_bank over the first nf - (Lmax(s) - L_j) frames with model j, at every window count; from 32
    windows on also against rp_mlp_forward_windows; and the zero-row rules"""
    got = set_logits[nf]
    pitch = max(M.n_win_of(nf, row) for row in M.SETS)
    assert got.shape == (M.S, M.SET_SIZE, pitch, M.LABEL_PITCH) and np.isfinite(got).all()
    compared = shared = 0
    for s, row in enumerate(M.SETS):
        nw, lm = M.n_win_of(nf, row), M.lmax_of(row)
        assert not got[s, :, nw:].any(), s                       # behind n_win_s, and every slot of a stream shorter than Lmax(s)
        for j, mi in enumerate(row):
            if mi < 0:
                assert not got[s, j].any(), (s, j)               # an empty slot
                continue
            L, nl = M.MODELS[mi][0], M.MODELS[mi][2]
            assert not got[s, j, :, nl:].any(), (s, j)           # behind the model's labels
            if nw == 0:
                continue
            head = rows[nf][s:s + 1, :nf - (lm - L)]
            want = ctx.mlp_forward_windows_bank(head, bank, np.array([mi], np.int32))
            assert want.shape == (1, nw, M.LABEL_PITCH)
            assert np.array_equal(got[s, j, :nw].view(np.uint32), want[0].view(np.uint32)), (s, j, mi, nw)
            compared += 1
            if nw >= 32:
                one = ctx.mlp_forward_windows(head, models[mi])[0]
                assert ctx.last_mlp_kernel() == WANT_KERNEL, ctx.last_mlp_kernel()
                assert one.shape == (nw, nl) and np.array_equal(got[s, j, :nw, :nl].view(np.uint32), one.view(np.uint32)), (s, j, mi, nw)
                shared += 1
    print("nf %d: %d slot rows compared, %d of them also against the shared-model call" % (nf, compared, shared))
    live = int((M.SETS >= 0).sum())
    short = sum(int((row >= 0).sum()) for row in M.SETS if M.lmax_of(row) == 195)
    assert compared == (live - short if nf == 120 else live)
    # (at 120 frames the row whose longest window is 96 frames has 25 windows: its three slots are not held against the shared-model call)
    assert shared == {300: live, 220: live - short, 195: live - short, 120: live - short - 3}[nf]
    if nf == 220:
        assert M.n_win_of(nf, M.SETS[1]) == 26
    if nf == 195:
        assert M.n_win_of(nf, M.SETS[2]) == 1
    if nf == 120:
        assert M.n_win_of(nf, M.SETS[1]) == 0 and nf > 30 and not got[1].any() and not got[8].any()


def test_pitch_precision_and_batch_invariance(ctx, bank, rows, set_logits):
    nf = 300
    got = set_logits[nf]
    wide = ctx.mlp_forward_windows_bank_sets(rows[nf], bank, M.SETS, win_pitch=got.shape[2] + 5)
    assert np.array_equal(wide[:, :, :got.shape[2]], got) and not wide[:, :, got.shape[2]:].any()
    assert np.array_equal(ctx.mlp_forward_windows_bank_sets(rows[nf], bank, M.SETS, precision="bf16"), got)
    perm = np.random.default_rng(2).permutation(M.S)
    again = ctx.mlp_forward_windows_bank_sets(rows[nf][perm], bank, M.SETS[perm], win_pitch=got.shape[2])
    assert np.array_equal(again, got[perm])
    # duplicates change nothing: [a, a, b] holds the rows of a twice
    assert np.array_equal(got[5, 0], got[5, 1])


@pytest.fixture(scope="module")
def pcm():
    return M.pcm().astype(np.float32)


def f32(b):
    return float(np.array([b], np.uint32).view(np.float32)[0])


def records(det, dmod, dlab, n_det, s):
    return [(int(d["frame"]), int(d["window"]), int(d["counter"]), M.bits(d["avg_score"]), M.bits(d["score"]), (int(dmod[s][i]), int(dlab[s][i])))
            for i, d in enumerate(det[s][:n_det[s]])]


def test_set_size_one_equals_the_bank_calls(ra, ctx, bank, rows, pcm):
    """set_size 1: the logits of rp_mlp_forward_windows_bank bit for bit, the detections of rp_batch_detect_model_bank record for record"""
    idx = np.array([0, 3, 1, -1, 2, 4, 5, 1, 0], np.int32)
    for nf in (300, 220):
        a = ctx.mlp_forward_windows_bank_sets(rows[nf], bank, idx[:, None])
        b = ctx.mlp_forward_windows_bank(rows[nf], bank, idx)
        assert a.shape == (M.S, 1) + b.shape[1:] and np.array_equal(a[:, 0].view(np.uint32), b.view(np.uint32))
    fired = 0
    for c in CONFIGS[:2]:
        cfg = config(ra, *c)
        det, dmod, dlab, n_det = ctx.batch_detect_model_bank_sets(pcm, bank, idx[:, None], cfg, max_det=16)
        wdet, wlab, wn = ctx.batch_detect_model_bank(pcm, bank, idx, cfg, max_det=16)
        assert np.array_equal(n_det, wn)
        for s in range(M.S):
            n = int(wn[s])
            assert det[s][:n].tobytes() == wdet[s][:n].tobytes(), s
            assert list(dlab[s][:n]) == list(wlab[s][:n]) and (dmod[s][:n] == idx[s]).all(), s
            assert not det[s][n:].tobytes().strip(b"\0") and (dmod[s][n:] == 0).all() and (dlab[s][n:] == -1).all()
            fired += n
    assert fired >= 10, fired


@pytest.mark.parametrize("case", range(len(CONFIGS)))
def test_detections_equal_the_host_fold(ra, ctx, bank, pcm, case):
    """the detection records of rp_batch_detect_model_bank_sets are exactly those of the host fold of the logits the sets call gives for the
    same frames: per window the best passing proposal with the first slot of equals, then the state machine with the label"""
    threshold, avg_threshold, vad, eager, min_scores = CONFIGS[case]
    cfg = config(ra, threshold, avg_threshold, vad, eager, min_scores)
    rc = R.Cfg(threshold=threshold, avg_threshold=avg_threshold, min_scores=min_scores, eager=eager, vad_mode=vad)
    mfcc = ctx.mfcc(pcm, M.K)
    nf = mfcc.shape[1]
    logits = ctx.mlp_forward_windows_bank_sets(mfcc, bank, M.SETS)
    det, dmod, dlab, n_det = ctx.batch_detect_model_bank_sets(pcm, bank, M.SETS, cfg, max_det=16)
    total, by_slot0, by_later, mixed, worst = 0, 0, 0, 0, 0.0
    for s, row in enumerate(M.SETS):
        want = M.fold_ref(logits[s], row, nf, rc, mfcc=mfcc[s])
        got = records(det, dmod, dlab, n_det, s)
        print("stream %d %s: %s" % (s, list(row), [(g[0], g[2], g[5]) for g in got]))
        # frame, window, counter, winner and label exactly; the two scores within 1e-6: the host evaluates the formula with its own exp, the
        # device with expf (the figure tests/test_gpu_nn_decide.py holds device scores to)
        assert [g[:3] + g[5:] for g in got] == [w[:3] + w[5:] for w in want], (s, got, want)
        for g, w in zip(got, want):
            worst = max(worst, abs(f32(g[3]) - float(w[3])), abs(f32(g[4]) - float(w[4])))
        assert all(d["stream"] == s for d in det[s][:n_det[s]])
        # `window`: where the best window of the detection starts, Lmax(s) - 1 frames before the frame that proposed it
        assert all(0 <= g[1] <= g[0] - M.lmax_of(row) for g in got)
        live = [mi for mi in row if mi >= 0]
        for g in got:
            assert g[5][0] in live and 0 <= g[5][1] < M.MODELS[g[5][0]][2] and g[5][1] != M.NONE_INDEX[g[5][0]]
            total += 1
            by_slot0 += g[5][0] == live[0]
            by_later += g[5][0] != live[0]
            mixed += len({M.MODELS[mi][0] for mi in live}) > 1
    print("case %d: %d detections, %d won by the first live slot, %d by a later one, %d in rows of different windows" % (case, total, by_slot0, by_later, mixed))
    print("worst score difference against the host formula %.3g" % worst)
    assert worst <= 1e-6
    assert not n_det[4]
    # the comparison is not empty (the counts the CPU design run gave with the oracle's forward: 21 and 35 detections without VAD)
    if vad is None:
        assert total >= 10 and by_slot0 >= 5
    if case == 1:
        assert by_later >= 2 and mixed >= 3


def test_twins_report_the_first_slot(ra, ctx, bank, pcm):
    """two bank indices holding the same parameters score the same: the first slot wins, in both orders"""
    cfg = config(ra, *CONFIGS[0])
    det, dmod, dlab, n_det = ctx.batch_detect_model_bank_sets(pcm, bank, M.SETS, cfg, max_det=16)
    assert n_det[6] >= 2 and n_det[7] >= 2
    assert (dmod[6][:n_det[6]] == M.SETS[6][0]).all() and (dmod[7][:n_det[7]] == M.SETS[7][0]).all()
    # and the same audio under both orders gives the same records but for the index
    both = np.stack([pcm[6], pcm[6]])
    d2, m2, l2, n2 = ctx.batch_detect_model_bank_sets(both, bank, np.array([[0, 5, -1], [5, 0, -1]], np.int32), cfg, max_det=16)
    assert n2[0] == n2[1] and n2[0] >= 2
    for a, b in zip(d2[0][:n2[0]], d2[1][:n2[1]]):
        assert all(a[f] == b[f] for f in ("frame", "window", "counter")) and a["score"].tobytes() == b["score"].tobytes()
    assert (m2[0][:n2[0]] == 0).all() and (m2[1][:n2[1]] == 5).all()


def test_indices(ra, ctx, bank, rows, set_logits, pcm):
    """host arrays: an index outside [-1, W) is an error that names the stream and the slot, nothing written; device arrays: the kernels
    treat it as -1"""
    import torch
    nf = 300
    got = set_logits[nf]
    idx = M.SETS.copy()
    idx[5, 2] = bank.W
    out = np.full(got.shape, 7.0, np.float32)
    L = ra.load_library()
    assert L.rp_mlp_forward_windows_bank_sets(ctx._h, bank._h, idx.ctypes.data, M.SET_SIZE, rows[nf].ctypes.data, M.S, nf, 0, out.ctypes.data, got.shape[2]) < 0
    msg = L.rp_last_error().decode()
    assert "stream 5, slot 2" in msg and "model index %d is outside the bank" % bank.W in msg and (out == 7.0).all()
    cfg = config(ra, *CONFIGS[0])
    with pytest.raises(ra.RustpotterError, match="stream 5, slot 2"):
        ctx.batch_detect_model_bank_sets(pcm, bank, idx, cfg)
    idx[5, 2] = -2
    with pytest.raises(ra.RustpotterError, match="stream 5, slot 2"):
        ctx.mlp_forward_windows_bank_sets(rows[nf], bank, idx)
    # device pointers: index W and -7 act as -1
    dctx = ra.BatchContext(device=0, host_pointers=False)
    dbank = ra.ModelBank(dctx, models=[ra.Model(dctx, ws, bs) for ws, bs in M.bank_weights()], none_index=M.NONE_INDEX)
    idx = M.SETS.copy()
    idx[5, 2], idx[1, 1] = bank.W, -7       # row 5 becomes [1, 1, -1], row 1 [0, -1, -1]
    clean = M.SETS.copy()
    clean[5, 2], clean[1, 1] = -1, -1
    want = ctx.mlp_forward_windows_bank_sets(rows[nf], bank, clean)
    pitch = nf - 30 + 1   # the largest window count any model of the bank has
    x, di = torch.from_numpy(rows[nf]).cuda(), torch.from_numpy(idx).cuda()
    dout = torch.full((M.S, M.SET_SIZE, pitch, M.LABEL_PITCH), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dctx.mlp_forward_windows_bank_sets_dev(dbank, di.data_ptr(), M.SET_SIZE, x.data_ptr(), M.S, nf, "f32", dout.data_ptr(), pitch)
    with pytest.raises(ra.RustpotterError, match="win_pitch"):
        dctx.mlp_forward_windows_bank_sets_dev(dbank, di.data_ptr(), M.SET_SIZE, x.data_ptr(), M.S, nf, "f32", dout.data_ptr(), pitch - 1)
    dctx.synchronize()
    dgot = dout.cpu().numpy()
    assert np.array_equal(dgot[:, :, :want.shape[2]], want) and not dgot[:, :, want.shape[2]:].any()
    # detection on device pointers: the records of the host-pointer call with the cleaned rows
    cfg = config(ra, *CONFIGS[1])
    wdet, wmod, wlab, wn = ctx.batch_detect_model_bank_sets(pcm, bank, clean, cfg, max_det=16)
    p = torch.from_numpy(pcm).cuda()
    det = torch.zeros((M.S, 16, wdet.dtype.itemsize), dtype=torch.uint8, device="cuda")
    dm, dl = torch.zeros((M.S, 16), dtype=torch.int32, device="cuda"), torch.zeros((M.S, 16), dtype=torch.int32, device="cuda")
    dn = torch.zeros(M.S, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dctx.batch_detect_model_bank_sets_dev(p.data_ptr(), 3, M.S, pcm.shape[1], pcm.shape[1], dbank, di.data_ptr(), M.SET_SIZE, cfg, "f32", det.data_ptr(),
                                          dm.data_ptr(), dl.data_ptr(), dn.data_ptr(), 16)
    dctx.synchronize()
    assert np.array_equal(dn.cpu().numpy(), wn) and wn.sum() >= 10
    assert det.cpu().numpy().tobytes() == wdet.tobytes()
    assert np.array_equal(dm.cpu().numpy(), wmod) and np.array_equal(dl.cpu().numpy(), wlab)


def test_refusals_and_the_empty_bank(ra, ctx, bank, rows, pcm):
    """win_pitch, precision, set_size, the empty bank and a foreign context: as rp_batch_detect_model_bank"""
    nf = 300
    cfg = config(ra, *CONFIGS[0])
    pitch = max(M.n_win_of(nf, row) for row in M.SETS)
    with pytest.raises(ra.RustpotterError, match="win_pitch %d is smaller than the largest window count of the call, %d" % (pitch - 1, pitch)):
        ctx.mlp_forward_windows_bank_sets(rows[nf], bank, M.SETS, win_pitch=pitch - 1)
    for prec in ("f32_fast", "f32_strict"):
        with pytest.raises(ra.RustpotterError, match="RP_MLP_F32_FAST and RP_MLP_F32_STRICT"):
            ctx.mlp_forward_windows_bank_sets(rows[nf], bank, M.SETS, precision=prec)
        with pytest.raises(ra.RustpotterError, match="RP_MLP_F32_FAST and RP_MLP_F32_STRICT"):
            ctx.batch_detect_model_bank_sets(pcm, bank, M.SETS, cfg, precision=prec)
    nine = np.full((M.S, 9), -1, np.int32)
    with pytest.raises(ra.RustpotterError, match=r"set_size 9 is outside 1 \.\. 8 \(RP_MODEL_SET_MAX\)"):
        ctx.mlp_forward_windows_bank_sets(rows[nf], bank, nine)
    with pytest.raises(ra.RustpotterError, match="RP_MODEL_SET_MAX"):
        ctx.batch_detect_model_bank_sets(pcm, bank, nine, cfg)
    eight = np.full((M.S, 8), -1, np.int32)
    eight[:, 7] = 0
    wide = ctx.mlp_forward_windows_bank_sets(rows[nf], bank, eight)
    first = ctx.mlp_forward_windows_bank_sets(rows[nf], bank, eight[:, 7:])
    assert not wide[:, :7].any() and np.array_equal(wide[:, 7], first[:, 0])
    empty = ra.ModelBank(ctx, models=[])
    none = np.full((M.S, M.SET_SIZE), -1, np.int32)
    assert ctx.mlp_forward_windows_bank_sets(rows[nf], empty, none).shape == (M.S, M.SET_SIZE, 0, 0)
    det, dmod, dlab, n_det = ctx.batch_detect_model_bank_sets(pcm, empty, none, cfg)
    assert not n_det.any() and not det["frame"].any() and not dmod.any() and not dlab.any()
    with pytest.raises(ra.RustpotterError, match="stream 0, slot 0"):
        ctx.mlp_forward_windows_bank_sets(rows[nf], empty, np.zeros((M.S, M.SET_SIZE), np.int32))
    other = ra.BatchContext(device=0, host_pointers=True)
    with pytest.raises(ra.RustpotterError, match="the bank belongs to another context"):
        other.mlp_forward_windows_bank_sets(rows[nf], bank, M.SETS)
    with pytest.raises(ra.RustpotterError, match="the bank belongs to another context"):
        other.batch_detect_model_bank_sets(pcm, bank, M.SETS, cfg)
    # a row of all -1 and the whole call of them: a detector without wakewords
    det, dmod, dlab, n_det = ctx.batch_detect_model_bank_sets(pcm, bank, none, cfg)
    assert not n_det.any()
