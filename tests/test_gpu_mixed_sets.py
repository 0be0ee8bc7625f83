"""Mixed sets over whole recordings (rp_batch_detect_mixed_sets, rp_frontend_batch_mixed_sets; mixed_targets_kernel, scan_mixed_set_kernel over
the rows of dtw_set_kernel and nn_score_model_set_kernel): stream s holds wakeword references of a wakeword bank AND models of a model bank,
as one Rustpotter with add_wakeword of both kinds -- one window of Lmax(s) frames over both rows, one countdown, one partial detection, the
best passing score winning, references before models of equals.
Yardstick: oracle.rp_oracle.Detector with add_ref per live reference slot, then add_model per live model slot, fed chunk by chunk
(tests/mixed_set_cases.py).  The chunk a detection is emitted in, its counter, the winner's kind, index in its own bank and label are exact;
reference scores within 1e-5 (relative, the bar of tests/test_gpu_bank_sets.py), model scores within 2e-6.  The
oracle reports no frame or window: the frame must lie in the oracle's chunk and the window inside the stream, Lmax(s) frames long, at or
before that frame; where two calls of the library are compared (device pointers, 130 streams, the degenerate rows) every field is exact.
Base configuration: thresholds 0.5 / 0.3, eager with min_scores 2 -- with windows of up to 207 frames in 396 a countdown of Lmax / 2 seldom
runs out, so the plain configuration (min_scores 5, not eager) reports little; it is one of the further configurations."""
import ctypes as C

import numpy as np
import pytest

import mixed_set_cases as X
import model_set_cases as M
from oracle import rp_oracle as orc

pytestmark = pytest.mark.gpu
MAX_DET = 16


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


def make_banks(ra, c):
    bank = ra.WakewordBank(c, wakewords=X.bank_wakewords())
    mbank = ra.ModelBank(c, models=[ra.Model(c, ws, bs) for ws, bs in M.bank_weights()], none_index=M.NONE_INDEX)
    return bank, mbank


@pytest.fixture(scope="module")
def banks(ra, ctx):
    bank, mbank = make_banks(ra, ctx)
    assert bank.max_lens == list(X.REF_LENS) and mbank.train_sizes == [m[0] for m in M.MODELS]
    return bank, mbank


@pytest.fixture(scope="module")
def pcm():
    return X.pcm()


def config(ra, c):
    cfg = ra.DetectorConfig()
    cfg.threshold, cfg.avg_threshold, cfg.eager, cfg.min_scores = c.threshold, c.avg_threshold, c.eager, c.min_scores
    cfg.band_size = c.band_size
    if c.vad_mode:
        cfg.vad_mode = {"easy": ra.VADMode.Easy}[c.vad_mode]
    return cfg


def records(det, dww, dlab, n_det, s):
    """-> [(frame, window, counter, score bits, avg bits, index in its own bank, label)]"""
    assert 0 <= n_det[s] <= det.shape[1]
    assert all(d["stream"] == s for d in det[s][:n_det[s]])
    assert not det[s][n_det[s]:].tobytes().strip(b"\0") and (dww[s][n_det[s]:] == 0).all() and (dlab[s][n_det[s]:] == -1).all()
    return [(int(d["frame"]), int(d["window"]), int(d["counter"]), M.bits(d["score"]), M.bits(d["avg_score"]), int(dww[s][i]), int(dlab[s][i]))
            for i, d in enumerate(det[s][:n_det[s]])]


def detect(ctx, banks, x, ref_rows, model_rows, cfg, **kw):
    det, dww, dlab, n_det = ctx.batch_detect_mixed_sets(x, banks[0], ref_rows, banks[1], model_rows, cfg, max_det=MAX_DET, **kw)
    return [records(det, dww, dlab, n_det, s) for s in range(len(x))]


def f32(b):
    return float(np.array([b], np.uint32).view(np.float32)[0])


def same_as_oracle(s, ref_row, model_row, got, want, nf):
    """chunk, counter, kind, bank index and label exact; the window inside the stream; scores at the two families' bars"""
    assert len(got) == len(want), (s, got, want)
    L = X.lmax_of(ref_row, model_row)
    for g, w in zip(got, want):
        chunk, kind, idx, label, score, avg, counter = w
        assert g[0] // 3 + 1 == chunk and g[2] == counter and 0 <= g[1] <= g[0] - L + 1 and g[0] < nf, (s, g, w)
        assert (g[6] >= 0) == (kind == "model") and g[5] == idx and g[6] == label, (s, g, w)
        sc, av = f32(g[3]), f32(g[4])
        print("stream %d chunk %d %s %d label %d: score %.7f (oracle %.7f) avg %.7f (oracle %.7f)" % (s, chunk, kind, idx, label, sc, score, av, avg))
        if kind == "model":
            assert abs(sc - float(score)) <= 2e-6 and abs(av - float(avg)) <= 2e-6, (s, g, w)
        else:
            assert abs(sc - float(score)) <= 1e-5 * float(score), (s, g, w)
            assert (av == 0) if avg == 0 else abs(av - float(avg)) <= 1e-5 * float(avg), (s, g, w)


_ORACLE = {}


def oracle_rows(c, x=None, tag="rows"):
    """the oracle's detections of every row of X.ROWS under the configuration c (an X.Cfg), computed once"""
    key = (tag, c.threshold, c.avg_threshold, c.min_scores, c.eager, c.band_size, c.vad_mode)
    if key not in _ORACLE:
        x = X.pcm() if x is None else x
        _ORACLE[key] = [X.oracle_detect(rr, mr, x[s], c) for s, (rr, mr, _, _) in enumerate(X.ROWS)]
    return _ORACLE[key]


@pytest.fixture(scope="module")
def base(ra, ctx, banks, pcm):
    """the rows under the base configuration with host pointers, computed once"""
    ctx.dtw_kernels()
    got = detect(ctx, banks, pcm, X.REF_ROWS, X.MODEL_ROWS, config(ra, X.Cfg()))
    assert ctx.dtw_kernels() == ["dtw_set_kernel"]   # the whole-recording call reports RP_DTW_KERNEL_BANK_SETS
    return got


# ---------------------------------------------------------------------------------------------- 1. the rows against the oracle

def test_inputs_show_the_feature(pcm):
    """on the ORACLE's output: references win beside live models, models beside live references, both kinds in one stream, and one
    detector over both rows differs from the union of a reference-only and a model-only detector over the same audio"""
    c = X.Cfg()
    want = oracle_rows(c)
    none = (-1, -1)
    alone = [(X.oracle_detect(rr, none, pcm[s], c), X.oracle_detect(none, mr, pcm[s], c)) for s, (rr, mr, _, _) in enumerate(X.ROWS)]
    print(X.check_inputs(want, alone))


def test_rows_against_the_oracle(base, pcm):
    want = oracle_rows(X.Cfg())
    nf = 3 * (pcm.shape[1] // 480) - 3
    for s, (rr, mr, _, _) in enumerate(X.ROWS):
        same_as_oracle(s, rr, mr, base[s], want[s], nf)
    assert sum(len(v) for v in base) >= 15 and not base[6]
    # `window` names the start of the winner's best window: Lmax(s) frames, whichever kind won
    for s, (rr, mr, _, _) in enumerate(X.ROWS):
        assert all(g[1] <= g[0] - X.lmax_of(rr, mr) + 1 for g in base[s])


def test_device_pointers(ra, base, pcm):
    """everything on the device; an index outside its bank counts as -1 on either side"""
    import torch
    dctx = ra.BatchContext(device=0, host_pointers=False)
    dbanks = make_banks(ra, dctx)
    rr, mr = X.REF_ROWS.copy(), X.MODEL_ROWS.copy()
    rr[6, 0], rr[1, 1], mr[6, 1], mr[0, 0] = 3, -9, 6, 77      # rows 6, 1 and 0 hold -1 there
    p = torch.from_numpy(pcm).cuda()
    dr, dm = torch.from_numpy(rr).cuda(), torch.from_numpy(mr).cuda()
    det = torch.zeros((X.S, MAX_DET, np.dtype(ra.api.DET_DTYPE).itemsize), dtype=torch.uint8, device="cuda")
    dw, dl = torch.full((X.S, MAX_DET), 7, dtype=torch.int32, device="cuda"), torch.full((X.S, MAX_DET), 7, dtype=torch.int32, device="cuda")
    dn = torch.zeros(X.S, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dctx.batch_detect_mixed_sets_dev(p.data_ptr(), 3, X.S, pcm.shape[1], pcm.shape[1], dbanks[0], dr.data_ptr(), 2, dbanks[1], dm.data_ptr(), 2,
                                     config(ra, X.Cfg()), "f32", det.data_ptr(), dw.data_ptr(), dl.data_ptr(), dn.data_ptr(), MAX_DET)
    dctx.synchronize()
    d = np.frombuffer(det.cpu().numpy().tobytes(), dtype=ra.api.DET_DTYPE).reshape(X.S, MAX_DET)
    got = [records(d, dw.cpu().numpy(), dl.cpu().numpy(), dn.cpu().numpy(), s) for s in range(X.S)]
    assert got == base


# ---------------------------------------------------------------------------------------------- 2. the degenerate rows, bit for bit

def test_one_side_absent_equals_the_family_call(ra, ctx, banks, pcm):
    """every model slot -1, model_set_size 0 / NULL: rp_batch_detect_bank_sets; every reference slot -1, ref_set_size 0 / NULL:
    rp_batch_detect_model_bank_sets -- record for record, bit for bit"""
    bank, mbank = banks
    none = np.full((X.S, 2), -1, np.int32)
    fired = 0
    for c in (X.Cfg(), X.Cfg(min_scores=5, eager=False), X.Cfg(vad_mode="easy")):
        cfg = config(ra, c)
        wdet, wdw, wn = ctx.batch_detect_bank_sets(pcm, bank, X.REF_ROWS, cfg, max_det=MAX_DET)[:3]
        want = [[r[:6] + (-1,) for r in records(wdet, wdw, np.full_like(wdw, -1), wn, s)] for s in range(X.S)]
        assert detect(ctx, banks, pcm, X.REF_ROWS, none, cfg) == want
        assert detect(ctx, banks, pcm, X.REF_ROWS, None, cfg) == want
        assert detect(ctx, banks, pcm, X.REF_ROWS, np.zeros((X.S, 0), np.int32), cfg) == want
        fired += sum(len(v) for v in want)
        mdet, mdw, mdl, mn = ctx.batch_detect_model_bank_sets(pcm, mbank, X.MODEL_ROWS, cfg, max_det=MAX_DET)
        want = [records(mdet, mdw, mdl, mn, s) for s in range(X.S)]
        assert detect(ctx, banks, pcm, none, X.MODEL_ROWS, cfg) == want
        assert detect(ctx, banks, pcm, None, X.MODEL_ROWS, cfg) == want
        fired += sum(len(v) for v in want)
    assert fired >= 30, fired


# ---------------------------------------------------------------------------------------------- 3. shorter than Lmax(s)

def test_a_stream_shorter_than_its_window(ra, ctx, banks):
    """The 42-frame reference beside the 195-frame model, U from the first chunk on, eager with min_scores 1.  65 chunks are 192 frames:
    shorter than Lmax = 195 although the reference alone fires on them -- nothing.  66 chunks are 195 frames, exactly one window: it
    proposes and no frame follows that could report it -- nothing.  67 chunks: the frame behind that one window reports it, window 0,
    counter 1 (the model wins it, by the oracle).  All three as the oracle says."""
    rr, mr = np.array([[0, -1]], np.int32), np.array([[3, -1]], np.int32)
    c = X.Cfg(min_scores=1)
    cfg = config(ra, c)
    u = X.utterance()
    got = {}
    for chunks in (65, 66, 67):
        x = u[None, :chunks * 480]
        nf = 3 * chunks - 3
        got[chunks] = detect(ctx, banks, x, rr, mr, cfg)[0]
        same_as_oracle(0, rr[0], mr[0], got[chunks], X.oracle_detect(rr[0], mr[0], x[0], c), nf)
    assert not got[65] and not got[66]
    assert len(got[67]) == 1 and got[67][0][:3] == (195, 0, 1)
    alone = detect(ctx, banks, u[None, :65 * 480], rr, None, cfg)[0]
    assert alone and alone[0][5] == 0


# ---------------------------------------------------------------------------------------------- 4. several workgroups

def test_130_streams(ra, ctx, banks, pcm, base):
    """two scan workgroups and a partial one: the rows repeated, every stream equal to its copy in the small call bit for bit"""
    rep = np.arange(130) % X.S
    got = detect(ctx, banks, pcm[rep], X.REF_ROWS[rep], X.MODEL_ROWS[rep], config(ra, X.Cfg()))
    for s in range(130):
        assert got[s] == base[rep[s]], s


# ---------------------------------------------------------------------------------------------- 5. further configurations

@pytest.mark.parametrize("name,kw", [("vad", dict(vad_mode="easy")), ("eager1", dict(min_scores=1)), ("min5", dict(min_scores=5, eager=False)),
                                     ("band3", dict(band_size=3)), ("band6", dict(band_size=6))])
def test_configurations_against_the_oracle(ra, ctx, banks, pcm, name, kw):
    c = X.Cfg(**kw)
    want = oracle_rows(c)
    got = detect(ctx, banks, pcm, X.REF_ROWS, X.MODEL_ROWS, config(ra, c))
    nf = 3 * (pcm.shape[1] // 480) - 3
    for s, (rr, mr, _, _) in enumerate(X.ROWS):
        same_as_oracle(s, rr, mr, got[s], want[s], nf)
    kinds = {w[1] for v in want for w in v}
    print(name, [[(w[0], w[1], w[2]) for w in v] for v in want])
    # (under the VAD the quiet stretches in front of U never count as voice: only models report)
    assert kinds == ({"model"} if name == "vad" else {"ref", "model"}), kinds


# ---------------------------------------------------------------------------------------------- 6. the front end

def test_frontend_against_the_oracle(ra, banks, ctx):
    """rp_frontend_batch_mixed_sets against oracle.frontend_stream per stream, as uint32: a stream whose model carries the larger rms_level,
    one whose reference does, one with every level NaN (gain 1), one without a live slot (gain 1), one side absent; the window is
    max(Lmax(s) / 3, 1) chunk levels over both rows"""
    from test_gpu_bank_filters import bits, varying_noise
    bank, mbank = make_banks(ra, ctx)
    ref_levels = np.array([0.02, float("nan"), 0.06], np.float32)
    model_levels = np.array([0.05, 0.01, float("nan"), 0.03, float("nan"), 0.09], np.float32)
    bank.set_rms_levels(ref_levels)
    mbank.set_rms_levels(model_levels)
    #        refs      models     level  Lmax
    plan = [((0, -1), (0, 3), 0.05, 195),      # the model's level is the larger one; the window comes from another slot
            ((2, 0), (1, -1), 0.06, 207),      # the reference's
            ((1, -1), (2, 4), None, 195),      # every level NaN: gain 1
            ((-1, -1), (-1, -1), None, 0),     # no live slot: gain 1
            ((0, 1), (5, -1), 0.09, 120),      # NaN beside real levels is ignored
            ((-1, 0), (-1, -1), 0.02, 42)]
    n, nc = len(plan), 90
    x = varying_noise(n, nc, np.random.default_rng(5), silent=None)
    f = ra.FiltersConfig()
    f.gain_normalizer.enabled, f.gain_normalizer.min_gain, f.gain_normalizer.max_gain = True, 0.3, 2.0
    f.band_pass.enabled, f.band_pass.low_cutoff, f.band_pass.high_cutoff = True, 120.0, 900.0
    rr, mr = np.array([p[0] for p in plan], np.int32), np.array([p[1] for p in plan], np.int32)
    out, rms, gains = ctx.frontend_batch_mixed_sets(x, f, bank, rr, mbank, mr)
    for s, (_, _, level, lmax) in enumerate(plan):
        assert X.lmax_of(plan[s][0], plan[s][1]) == lmax
        if level is None:
            want = orc.frontend_stream(x[s], band_pass=True, low_cutoff=120.0, high_cutoff=900.0)
            assert (gains[s] == 1.0).all()
        else:
            want = orc.frontend_stream(x[s], gain_normalizer=True, min_gain=0.3, max_gain=2.0, rms_level_ref=float(np.float32(level)),
                                       window_size=max(lmax // 3, 1), band_pass=True, low_cutoff=120.0, high_cutoff=900.0)
            assert np.mean(want[2] != 1.0) > 0.3
        for name, a, b in (("rms", rms[s], want[1]), ("gains", gains[s], want[2]), ("pcm", out[s], want[0])):
            assert np.array_equal(bits(a), bits(b)), (s, name)
    # one side absent: the bits of the family's own call
    a = ctx.frontend_batch_mixed_sets(x, f, bank, rr, mbank, None)
    b = ctx.frontend_bank_sets(x, f, bank, rr)
    assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, b))
    a = ctx.frontend_batch_mixed_sets(x, f, bank, None, mbank, mr)
    b = ctx.frontend_model_bank(x, f, mbank, mr)
    assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, b))


# ---------------------------------------------------------------------------------------------- 7. refusals and edges

def test_refusals_and_edges(ra, ctx, banks, pcm):
    bank, mbank = banks
    L = ra.load_library()
    cfg = config(ra, X.Cfg())
    c = cfg._c()
    x = np.ascontiguousarray(pcm[:2])
    rr, mr = np.ascontiguousarray(X.REF_ROWS[:2]), np.ascontiguousarray(X.MODEL_ROWS[:2])
    det = np.zeros((2, 4), dtype=ra.api.DET_DTYPE)
    dww, dlab, n_det = np.full((2, 4), 7, np.int32), np.full((2, 4), 7, np.int32), np.full(2, 7, np.int32)

    def call(bk=bank._h, mb=mbank._h, r=rr.ctypes.data, rn=2, m=mr.ctypes.data, mn=2, prec=0, max_det=4, context=ctx):
        return L.rp_batch_detect_mixed_sets(context._h, x.ctypes.data, 3, 2, x.shape[1], x.shape[1], bk, r, rn, mb, m, mn, C.byref(c), prec,
                                            det.ctypes.data, dww.ctypes.data, dlab.ctypes.data, n_det.ctypes.data, max_det)

    def refused(text, **kw):
        assert call(**kw) == -1 and text in L.rp_last_error().decode(), (kw, L.rp_last_error())

    assert call() == 0 and n_det[0] != 7
    dww[:], dlab[:], n_det[:] = 7, 7, 7
    five = ra.WakewordBank(ctx, wakewords=[([orc.synth_templates(3, 1, 40, 5)[0]], None, None, None)])
    refused("Usage of wakewords with different mfcc size is not supported, ignoring wakeword", bk=five._h)
    other = ra.BatchContext(device=0, host_pointers=True)
    obank, ombank = make_banks(ra, other)
    refused("the wakeword bank belongs to another context", bk=obank._h)
    refused("the model bank belongs to another context", mb=ombank._h)
    refused("the wakeword bank belongs to another context", context=other)
    for n in (9, -1):
        refused("ref_set_size %d is outside 0 .. 8 (RP_WAKEWORD_SET_MAX)" % n, rn=n)
        refused("model_set_size %d is outside 0 .. 8 (RP_MODEL_SET_MAX)" % n, mn=n)
    refused("null argument", r=None)
    refused("null argument", m=None)
    refused("null handle", bk=None)
    refused("null handle", mb=None)
    bad = rr.copy()
    bad[1, 1] = 3
    refused("stream 1, slot 1: wakeword index 3 is outside the bank (-1 .. 2)", r=bad.ctypes.data)
    bad = mr.copy()
    bad[1, 0] = -2
    refused("stream 1, slot 0: model index -2 is outside the bank (-1 .. 5)", m=bad.ctypes.data)
    refused("RP_MLP_F32_FAST", prec=3)
    refused("max_det must be >= 0", max_det=-1)
    with pytest.raises(ra.RustpotterError, match="is not built"):
        cfg8 = config(ra, X.Cfg(band_size=8))
        ctx.batch_detect_mixed_sets(x, bank, rr, mbank, mr, cfg8)
    assert (dww == 7).all() and (dlab == 7).all() and (n_det == 7).all(), "the refusals wrote nothing"
    # RP_MLP_BF16 computes the same
    assert detect(ctx, banks, x, rr, mr, cfg, precision="bf16") == detect(ctx, banks, x, rr, mr, cfg)
    # both banks empty: success, nothing reported, zeroed outputs
    ebank, embank = ra.WakewordBank(ctx, wakewords=[]), ra.ModelBank(ctx, models=[])
    none = np.full((2, 2), -1, np.int32)
    assert call(bk=ebank._h, mb=embank._h, r=none.ctypes.data, m=none.ctypes.data) == 0
    assert not n_det.any() and not det.tobytes().strip(b"\0") and not dww.any() and not dlab.any()
    # one empty bank beside a full one: that side is absent
    got = detect(ctx, (ebank, mbank), x, none, mr, cfg)
    assert got == detect(ctx, banks, x, None, mr, cfg) and any(got)
    # rows of all -1 over full banks
    assert not any(detect(ctx, banks, x, none, none, cfg))
    assert call() == 0, "the refusals left the context usable"
