"""What happens AFTER a wakeword model's logits -- the label rule, the two scores, the two gates, the per-stream "hot" flag, the label that
travels with a partial detection, the label gather behind the scan -- in its four copies on the product's side: nn_score_kernel
(rp_batch_detect_model, live batches with a shared model), nn_score_bank_kernel (rp_batch_detect_model_bank), nn_score_bank_stream_kernel
(live batches over a model bank) and the host loop of the single-stream Rustpotter.  The yardstick is tests/nn_decide_ref.py, restated from
the Rust source and pinned to the oracle on the CPU by tests/test_nn_decide_ref.py; it is applied to the DEVICE's own logits, so every
difference is a difference of this stage.

Steered models put chosen logits into it.  Constant models (last layer all-zero weights) answer their bias for every window: equal logits
(the LAST maximum; values equal to the label's left out of second_prob; nothing left: 0), thresholds at and one ulp above a score (>= in the
kernel, > -1 in the scan), a threshold of 0.2 below the 0.2689 of a row of zero logits (the rows behind a short stream's windows in a bank
call), a NaN logit.  Every window passes, so a stream reports only in eager mode and then resets and refills every few frames.  Moving
models (two logits that rise at different times) make detections whose best window carries another label than their first or last one --
the label a partial detection carries across calls.
Not driven: the +-0 ordering of total_cmp (tests/test_nn_decide_ref.py::test_minus_zero_cannot_leave_the_forward says why)."""
import numpy as np
import pytest

import nn_decide_ref as R
import rpw_py
from oracle import rp_oracle as orc

pytestmark = pytest.mark.gpu
F32 = np.float32
K = R.K
CHUNKS = R.MOVING_CHUNKS       # 3 s
NF = 3 * CHUNKS - 3            # MFCC frames of CHUNKS chunks
MAX_CHUNKS = 11                # per live call: 33 rows, past two 16-row tiles
MAX_DET = 40                   # no stream fills it: an L = 20 stream that fires on every window reports every 24 frames
CONST_THRESHOLD, CONST_AVG = 0.2, 0.2
TABLE = list(R.CONSTANT) + ["nan"]


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


def config(ra, threshold, avg_threshold, min_scores=1, eager=True):
    cfg = ra.DetectorConfig()
    cfg.threshold, cfg.avg_threshold, cfg.min_scores, cfg.eager = threshold, avg_threshold, min_scores, eager
    return cfg


def const_model(name, L=None, hidden=None):
    bias, none_index = R.constant_vector(name)
    shape = R.CONSTANT_SHAPES[name]
    return R.constant_model(bias, none_index, shape[0] if L is None else L, shape[1] if hidden is None else hidden, seed=len(name))


@pytest.fixture(scope="module")
def device_models(ra, ctx):
    """name -> (model dict, rp_model): every constant vector in its shape of CONSTANT_SHAPES, "moving0" / "moving1" """
    out = {}
    for name in R.CONSTANT_SHAPES:
        m = const_model(name)
        out[name] = (m, ra.Model(ctx, m["ws"], m["bs"]))
    for i, m in enumerate(R.moving_models()):
        out["moving%d" % i] = (m, ra.Model(ctx, m["ws"], m["bs"]))
    return out


def bits(x):
    return int(np.array(x, F32).view(np.uint32))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


def answers_bias(lg, bias):
    """every row of lg is the bias, bit for bit (a NaN entry: a NaN)"""
    nan = np.isnan(bias)
    return lg.shape[-1] == len(bias) and same_bits(lg[..., ~nan], np.broadcast_to(bias[~nan], lg[..., ~nan].shape)) and np.isnan(lg[..., nan]).all()


def gate_distance(lg, none_index, cfg):
    """how close the f64 score (and avg score) of any window comes to its gate"""
    d = np.inf
    for row in lg:
        f = R.decide_f64(row, none_index, cfg.score_ref, cfg.avg_threshold)
        if f is not None and np.isfinite(f[1]):
            d = min(d, abs(f[1] - float(F32(cfg.threshold))))
            if cfg.avg_threshold != 0.0:
                d = min(d, abs(f[2] - float(F32(cfg.avg_threshold))))
    return d


def check_stream(got, lg, L, none_index, cfg, tol=1e-6, first_frame=0):
    """got: [(frame, window, counter, score, avg_score, label)] of one stream; lg [n_win][labels]: the device's logits of its windows, row w
    the window that starts at frame first_frame + w.  detect_model_ref on them gives frame, window, counter and label exactly; the scores
    are within tol of the f64 formula on the f32 logits of the detection's window"""
    want = R.detect_model_ref(lg, L, none_index, cfg)
    assert [(g[0] - first_frame, g[1] - first_frame, g[2], g[5]) for g in got] == [(w[0], w[1], w[2], int(w[5])) for w in want], (got, want)
    worst = 0.0
    for g in got:
        f = R.decide_f64(lg[g[1] - first_frame], none_index, cfg.score_ref, cfg.avg_threshold)
        assert f[0] == g[5]
        worst = max(worst, abs(float(g[3]) - f[1]), abs(float(g[4]) - f[2]))
    assert worst <= tol, worst
    return len(want), worst


def unpack(det, dlab, n_det, s, max_det=MAX_DET):
    assert n_det[s] < max_det, (s, n_det[s])
    assert not det[s][n_det[s]:].tobytes().strip(b"\0"), "slots behind a stream's detections are zero"
    out = []
    for j in range(n_det[s]):
        d = det[s][j]
        assert d["stream"] == s
        out.append((int(d["frame"]), int(d["window"]), int(d["counter"]), F32(d["score"]), F32(d["avg_score"]), int(dlab[s][j])))
    return out


# ------------------------------------------------------------------ 1. whole recording, shared model
CONST_PCM_CHUNKS = 60     # 177 frames: S * n_win = 3 * 158 (L 20) or 3 * 138 (L 40), past 256 and no multiple of it


@pytest.mark.parametrize("avg_threshold", [0.0, CONST_AVG])
@pytest.mark.parametrize("name", TABLE)
def test_whole_recording_constant(ra, ctx, device_models, name, avg_threshold):
    """rp_batch_detect_model with a model that answers the table's vector: eager with min_scores 1 and 3 every stream reports what
    detect_model_ref reports on those logits; not eager nothing is reported (every window passes: the countdown never runs out).  S = 3
    (two blocks of nn_score_kernel, the second partial) and S = 1"""
    m, model = device_models[name]
    bias, none_index = R.constant_vector(name)
    L = m["train_size"]
    pcm = R.noise_pcm(3, CONST_PCM_CHUNKS)
    lg = ctx.mlp_forward_windows(ctx.mfcc(pcm, K), model)
    assert lg.shape[1] == 3 * CONST_PCM_CHUNKS - 3 - L + 1 and 3 * lg.shape[1] > 256 and (3 * lg.shape[1]) % 256 and lg.shape[1] < 256
    assert answers_bias(lg, bias), "a model whose last layer has zero weights answers its bias"
    fires = name != "nan" and R.CONSTANT[name][2] is not None
    for eager, min_scores in ((True, 1), (True, 3), (False, 1)):
        cfg = config(ra, CONST_THRESHOLD, avg_threshold, min_scores, eager)
        for S in (3, 1):
            det, dlab, n_det = ctx.batch_detect_model(pcm[:S], model, K, none_index, cfg, max_det=MAX_DET)
            for s in range(S):
                n, worst = check_stream(unpack(det, dlab, n_det, s), lg[s], L, none_index, cfg)
                assert (n >= 2) if (fires and eager) else n == 0, (name, eager, min_scores, n)
    if fires:
        want = R.expected_constant(name, avg_threshold)
        # the table's figures themselves (the last run reported nothing: one more, eager)
        det, dlab, n_det = ctx.batch_detect_model(pcm[:1], model, K, none_index, config(ra, CONST_THRESHOLD, avg_threshold), max_det=MAX_DET)
        d = unpack(det, dlab, n_det, 0)
        assert d and all(g[5] == want[0] and abs(float(g[3]) - want[1]) <= 1e-6 and abs(float(g[4]) - want[2]) <= 1e-6 for g in d), (d, want)


def test_hot_flag_is_not_left_behind(ra, ctx, device_models):
    """a call in which every stream fires, then on the same context a model that never fires ([a, a] with none 1; the none label alone):
    nothing is reported, and the firing call after it is what it was"""
    pcm = R.noise_pcm(3, CONST_PCM_CHUNKS)
    cfg = config(ra, CONST_THRESHOLD, CONST_AVG)
    first = ctx.batch_detect_model(pcm, device_models["aa_none0"][1], K, 0, cfg, max_det=MAX_DET)
    assert (first[2] >= 2).all()
    for name in ("aa_none1", "a_none0"):
        det, dlab, n_det = ctx.batch_detect_model(pcm, device_models[name][1], K, R.constant_vector(name)[1], cfg, max_det=MAX_DET)
        assert not n_det.any() and not det.tobytes().strip(b"\0")
    again = ctx.batch_detect_model(pcm, device_models["aa_none0"][1], K, 0, cfg, max_det=MAX_DET)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


@pytest.fixture(scope="module")
def moving_pcm():
    return R.moving_pcm()


def moving_streams(mi):
    return [s for s, m in enumerate(R.MOVING_STREAM_MODEL) if m == mi]


@pytest.fixture(scope="module")
def moving_whole(ra, ctx, device_models, moving_pcm):
    """(avg_threshold, eager, min_scores) -> per stream of the moving set the detections of rp_batch_detect_model with its model, checked
    against detect_model_ref on the device's logits"""
    out = {}
    for avg_threshold in (0.0, R.MOVING_AVG_THRESHOLD):
        for eager, min_scores in ((False, 1), (False, 3), (True, 3)):
            cfg = config(ra, R.MOVING_THRESHOLD, avg_threshold, min_scores, eager)
            per = [None] * R.MOVING_STREAMS
            for mi in range(len(R.MOVING)):
                m, model = device_models["moving%d" % mi]
                ss = moving_streams(mi)
                pcm = moving_pcm[ss]
                lg = ctx.mlp_forward_windows(ctx.mfcc(pcm, K), model)
                det, dlab, n_det = ctx.batch_detect_model(pcm, model, K, 0, cfg, max_det=MAX_DET)
                for i, s in enumerate(ss):
                    assert gate_distance(lg[i], 0, cfg) > 1e-5, "a window on a gate: the test's audio is badly chosen"
                    per[s] = unpack(det, dlab, n_det, i)
                    check_stream(per[s], lg[i], m["train_size"], 0, cfg)
            out[(avg_threshold, eager, min_scores)] = per
    return out


def test_whole_recording_moving(moving_whole):
    """rp_batch_detect_model on the moving set (the fixture holds every detection against the reference): 3 detections or more per stream,
    both labels, counters above 1"""
    for key, per in moving_whole.items():
        n = [len(p) for p in per]
        labels = {g[5] for p in per for g in p}
        print(key, n, sorted(labels))
        assert labels == {1, 2}
        if key[1:] == (False, 1):
            assert min(n) >= 3 and sum(g[2] >= 2 for p in per for g in p) >= 2


# ------------------------------------------------------------------ 2. a score on its threshold
def _equality(run):
    """run(threshold, avg_threshold) -> the first stream's detections [(frame, window, counter, score, avg, label)].  With the threshold ON
    the score the device reports the detections stay (>=), one ulp above there are none; the same for the avg threshold"""
    base = run(CONST_THRESHOLD, CONST_AVG)
    assert len(base) >= 2
    x, y = F32(base[0][3]), F32(base[0][4])
    assert all(bits(g[3]) == bits(x) and bits(g[4]) == bits(y) for g in base) and x != y
    key = lambda d: [(g[0], g[1], g[2], bits(g[3]), bits(g[4]), g[5]) for g in d]
    assert key(run(float(x), CONST_AVG)) == key(base)
    assert run(float(np.nextafter(x, F32(np.inf))), CONST_AVG) == []
    assert key(run(CONST_THRESHOLD, float(y))) == key(base)
    assert run(CONST_THRESHOLD, float(np.nextafter(y, F32(np.inf)))) == []


@pytest.mark.parametrize("path", ["shared", "bank", "live_bank", "live_shared"])
def test_threshold_equality(ra, ctx, device_models, path):
    """[a, a] with none 0: score f(0) = 0.2689, avg f(a)"""
    m, model = device_models["aa_none0"]
    pcm = R.noise_pcm(2, 30)
    bank = ra.ModelBank(ctx, models=[model], none_index=[0])
    idx = np.zeros(2, np.int32)

    def run(threshold, avg_threshold):
        cfg = config(ra, threshold, avg_threshold)
        if path == "shared":
            return unpack(*ctx.batch_detect_model(pcm, model, K, 0, cfg, max_det=MAX_DET), 0)
        if path == "bank":
            return unpack(*ctx.batch_detect_model_bank(pcm, bank, idx, cfg, max_det=MAX_DET), 0)
        if path == "live_bank":
            sb = ra.StreamBatch(ctx, None, cfg, 2, max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_model=idx)
        else:
            sb = ra.StreamBatch(ctx, None, cfg, 2, max_chunks_per_call=MAX_CHUNKS, wakewords=[{"model": model, "none_index": 0}], mfcc_size=K)
        return feed(sb, pcm, (4,))[0][0]

    _equality(run)


def rustpotter_run(ra, model, pcm, cfg):
    """the single-stream detector over 480-sample chunks -> [(chunk, RustpotterDetection)]; the model goes in as .rpw bytes"""
    rc = ra.RustpotterConfig()
    rc.detector = cfg
    rp = ra.Rustpotter(rc)
    rp.add_wakeword_from_buffer("w", rpw_py.dump_rpw_model(model["labels"], model["train_size"], K, model["m_type"], model["weights"]))
    out = []
    for c in range(len(pcm) // 480):
        r = rp.process_samples(pcm[c * 480:(c + 1) * 480])
        if r is not None:
            out.append((c, r))
    return out


def test_threshold_equality_rustpotter(ra):
    """the host loop, with the scores IT reports (std::exp on the host is not expf on the device)"""
    model = const_model("aa_none0", 20, (3,))
    pcm = R.noise_pcm(1, 20)[0]

    def run(threshold, avg_threshold):
        return [(c, 0, r.counter, r.score, r.avg_score, r.name) for c, r in rustpotter_run(ra, model, pcm, config(ra, threshold, avg_threshold))]

    _equality(run)


# ------------------------------------------------------------------ 3. / 4. the model bank, whole recordings and live
# the bank: constant and moving models, L 20 and 40, 1, 2, 3 and 32 labels, one layer and two
BANK = ["moving0", "moving1", "aa_none0", "baa_none0", "wide32_none0", "a_nonone", "aa_none1", "abc_none2", "cab_none0", "aa_nonone",
        "a_none0", "nan", "quiet"]
# streams:               moving0 moving1 aa_none0 baa wide32 (no model) a_nonone aa_none1 abc cab quiet nan a_none0
STREAM_MODEL = np.array([0, 1, 2, 3, 4, -1, 5, 6, 7, 8, 12, 11, 10], np.int32)
S = len(STREAM_MODEL)
BANK_CASES = [(CONST_THRESHOLD, 0.0, 1, True), (CONST_THRESHOLD, CONST_AVG, 3, True), (R.MOVING_THRESHOLD, R.MOVING_AVG_THRESHOLD, 1, False)]


@pytest.fixture(scope="module")
def bank(ra, ctx, device_models):
    assert S <= 13 and {device_models[n][0]["train_size"] for n in BANK} == {20, 40}
    assert {len(device_models[n][0]["labels"]) for n in BANK} == {1, 2, 3, 32}
    # the model bank takes one-layer models like any other
    b = ra.ModelBank(ctx, models=[device_models[n][1] for n in BANK], none_index=[device_models[n][0]["none_index"] for n in BANK])
    assert b.label_pitch == 32 and b.train_sizes == [device_models[n][0]["train_size"] for n in BANK]
    return b


@pytest.fixture(scope="module")
def bank_pcm(moving_pcm):
    pcm = R.noise_pcm(S, CHUNKS, seed=11)
    pcm[0], pcm[1] = moving_pcm[0], moving_pcm[1]     # a stream of each moving model hears ITS bursts
    return pcm


def bank_entry(device_models, mi):
    m = device_models[BANK[mi]][0]
    return m, m["train_size"], len(m["labels"]), m["none_index"]


@pytest.mark.parametrize("threshold,avg_threshold,min_scores,eager", BANK_CASES)
def test_model_bank_whole_recording(ra, ctx, device_models, bank, bank_pcm, threshold, avg_threshold, min_scores, eager):
    """rp_batch_detect_model_bank: every stream equals detect_model_ref on rp_mlp_forward_windows_bank's own rows for it, det_label included.
    The threshold of 0.2 lies below the 0.2689 a row of zero logits scores: the 20 such rows behind the windows of every L = 40 stream
    must not fire (the "quiet" model's own windows never do, so ANY detection of its stream comes from them); the stream without a model
    reports nothing.  (rp_batch_detect_model_bank takes no win_pitch: the call sizes its rows itself.)  The call runs twice on the
    context, first with every stream on a firing model: a hot flag left behind would show in the second"""
    cfg = config(ra, threshold, avg_threshold, min_scores, eager)
    rows = ctx.mlp_forward_windows_bank(ctx.mfcc(bank_pcm, K), bank, STREAM_MODEL)
    assert rows.shape == (S, NF - 20 + 1, 32)
    if eager:
        all_fire = np.full(S, 2, np.int32)
        _, _, n_first = ctx.batch_detect_model_bank(bank_pcm, bank, all_fire, cfg, max_det=MAX_DET)
        assert (n_first >= 2).all()
    det, dlab, n_det = ctx.batch_detect_model_bank(bank_pcm, bank, STREAM_MODEL, cfg, max_det=MAX_DET)
    fired = {}
    for s, mi in enumerate(STREAM_MODEL):
        got = unpack(det, dlab, n_det, s)
        if mi < 0:
            assert not got and not rows[s].any()
            continue
        m, L, nl, none_index = bank_entry(device_models, mi)
        nw = NF - L + 1
        assert not rows[s, nw:].any() and not rows[s, :, nl:].any() and (L == 20 or rows[s, nw:].shape[0] == 20)
        if BANK[mi].startswith("moving"):
            assert gate_distance(rows[s, :nw, :nl], none_index, cfg) > 1e-6, "a window on a gate: the test's audio is badly chosen"
        else:
            assert answers_bias(rows[s, :nw, :nl], R.constant_vector(BANK[mi])[0])
        assert all(g[1] < nw for g in got), (s, got)
        fired[BANK[mi]] = check_stream(got, rows[s, :nw, :nl], L, none_index, cfg)[0]
    print(fired)
    assert not any(fired[n] for n in ("aa_none1", "a_none0", "nan", "quiet")) and fired["moving0"] >= 3 and fired["moving1"] >= 3
    if eager:
        assert all(n >= 2 for name, n in fired.items() if name not in ("aa_none1", "a_none0", "nan", "quiet"))


def feed(sb, pcm, pieces, before_chunk=None, want_logits=False, max_det=MAX_CHUNKS + 2):
    """pcm [S][C * 480] through the batch in calls of pieces[0], pieces[1], ... chunks (cycled) -> per stream [(frame, window, counter,
    score, avg, label, index of the call that reported it)], and the logits of every call side by side, [S][3 C][label pitch]: column j is
    the window that ends at frame j - 3"""
    n_streams, total = pcm.shape[0], pcm.shape[1] // 480
    out, logits = [[] for _ in range(n_streams)], []
    c = k = 0
    while c < total:
        n = min(pieces[k % len(pieces)], total - c)
        if before_chunk is not None:
            before_chunk(c)
        det, dww, dlab, n_det = sb.process_multi(np.ascontiguousarray(pcm[:, c * 480:(c + n) * 480]), max_det=max_det)
        for s in range(n_streams):
            out[s] += [g + (k,) for g in unpack(det, dlab, n_det, s, max_det)]
            assert (dlab[s][n_det[s]:] == -1).all()
        if want_logits:
            logits.append(sb.logits())
            assert logits[-1].shape[:2] == (n_streams, 3 * n)
        c += n
        k += 1
    return out, (np.concatenate(logits, axis=1) if want_logits else None)


def live_key(per):
    return [[(g[0], g[1], g[2], bits(g[3]), bits(g[4]), g[5]) for g in p] for p in per]


def live_windows(lg, L, nl):
    """a live stream's logits [3 C][pitch] -> [n_win][nl], row w the window that starts at frame w (it ends at column w + L - 1 + 3)"""
    return lg[L + 2:, :nl]


@pytest.mark.parametrize("threshold,avg_threshold,min_scores,eager", BANK_CASES)
def test_model_bank_live(ra, ctx, device_models, bank, bank_pcm, threshold, avg_threshold, min_scores, eager):
    """a live batch over the bank, fed in calls of 1, of 3 / 1 / 2 and of 11 chunks: every stream equals detect_model_ref on the batch's
    own logits from its first full window on (the rows a stream does not read -- before that window, and while it refills after a reset,
    with ITS window length -- do not matter to the reference either); detections and score bits are the same for every cut.  Not eager,
    the moving models report detections whose best window was seen in an EARLIER call than the one that reports them, with that
    window's label and not the label of the windows of the reporting call"""
    cfg = config(ra, threshold, avg_threshold, min_scores, eager)
    runs = []
    for pieces in ((1,), (3, 1, 2), (MAX_CHUNKS,)):
        sb = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_model=STREAM_MODEL)
        runs.append(feed(sb, bank_pcm, pieces, want_logits=True))
    det, lg = runs[0]
    assert lg.shape == (S, 3 * CHUNKS, 32)
    fired, carried = {}, 0
    for s, mi in enumerate(STREAM_MODEL):
        if mi < 0:
            assert not det[s] and not lg[s].any()
            continue
        m, L, nl, none_index = bank_entry(device_models, mi)
        rows = live_windows(lg[s], L, nl)
        assert rows.shape == (NF - L + 1, nl) and not lg[s, :, nl:].any()
        if not BANK[mi].startswith("moving"):
            assert answers_bias(rows[:1], R.constant_vector(BANK[mi])[0])
        fired[BANK[mi]] = check_stream([g[:6] for g in det[s]], rows, L, none_index, cfg)[0]
        for g in det[s]:    # calls of one chunk: call k holds frames 3 k - 3 .. 3 k - 1
            seen = (g[1] + L - 1 + 3) // 3
            here = [R.get_label(rows[w]) for w in range(3 * g[6] - 3 - L + 1, min(3 * g[6] - L + 1, len(rows)))]
            carried += seen < g[6] and g[5] not in here
    for other, _ in runs[1:]:
        assert live_key(other) == live_key(det)
    print(fired, "carried labels:", carried)
    assert not any(fired[n] for n in ("aa_none1", "a_none0", "nan", "quiet"))
    if eager:
        assert all(n >= 2 for name, n in fired.items() if name not in ("aa_none1", "a_none0", "nan", "quiet"))
    else:
        assert fired["moving0"] >= 3 and fired["moving1"] >= 3 and carried >= 2


def test_model_bank_live_set_models(ra, ctx, device_models, bank, bank_pcm):
    """rp_stream_batch_set_models between two calls: a firing stream goes from an L = 20 model to an L = 40 model (and one the other way).
    From that chunk on it equals a fresh batch started there -- and the reference on its logits, whose refill now takes the OTHER window
    length; before, and on every other stream, the uninterrupted run"""
    cfg = config(ra, CONST_THRESHOLD, CONST_AVG)
    half = 31
    new = {2: 3, 9: 7}      # stream 2: aa_none0 (L 20) -> baa_none0 (L 40); stream 9: cab_none0 (L 40) -> abc_none2 (L 20)
    assert all(bank.train_sizes[STREAM_MODEL[s]] != bank.train_sizes[mi] for s, mi in new.items())
    whole, _ = feed(ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_model=STREAM_MODEL), bank_pcm, (5, 2))
    sb = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_model=STREAM_MODEL)

    def at(c):
        if c == half:
            for s, mi in new.items():
                sb.set_models(s, np.array([mi], np.int32))

    pieces = (5, 2, 5, 2, 5, 2, 5, 2, 3) + (5, 2) * 20   # a call boundary at chunk 31
    det, lg = feed(sb, bank_pcm, pieces, before_chunk=at, want_logits=True)
    for s in range(S):
        if s not in new:
            assert live_key([det[s]]) == live_key([whole[s]]), s
            continue
        cut = 3 * half - 3      # the first frame of chunk `half`
        assert live_key([[g for g in det[s] if g[0] < cut]]) == live_key([[g for g in whole[s] if g[0] < cut]]), s
        m, L, nl, none_index = bank_entry(device_models, new[s])
        fresh_sb = ra.StreamBatch(ctx, None, cfg, 1, max_chunks_per_call=MAX_CHUNKS, model_bank=bank, stream_model=np.array([new[s]], np.int32))
        fresh, _ = feed(fresh_sb, bank_pcm[s:s + 1, half * 480:], (5, 2))
        after = [g for g in det[s] if g[0] >= cut]
        moved = [(g[0] + 3 * half, g[1] + 3 * half) + g[2:6] for g in fresh[0]]
        assert live_key([after]) == live_key([moved]) and len(after) >= 2, (s, after, moved)
        # the reference on the stream's logits from the change on: a stream that starts at chunk `half`
        rows = live_windows(lg[s, 3 * half:], L, nl)
        check_stream([g[:6] for g in after], rows, L, none_index, cfg, first_frame=3 * half)


# ------------------------------------------------------------------ 5. live, shared model
@pytest.mark.parametrize("name", TABLE)
def test_live_shared_constant(ra, ctx, device_models, name):
    """rp_stream_batch_new_multi with one model (nn_score_kernel behind the in-place forward; no logits getter): the reference on the BIAS,
    exactly"""
    m, model = device_models[name]
    bias, none_index = R.constant_vector(name)
    L = m["train_size"]
    pcm = R.noise_pcm(2, CONST_PCM_CHUNKS)
    lg = np.tile(bias, (3 * CONST_PCM_CHUNKS - 3 - L + 1, 1))
    fires = name != "nan" and R.CONSTANT[name][2] is not None
    for avg_threshold, min_scores, eager, pieces in ((0.0, 1, True, (1,)), (CONST_AVG, 3, True, (3, 1, 2)), (CONST_AVG, 1, False, (MAX_CHUNKS,))):
        cfg = config(ra, CONST_THRESHOLD, avg_threshold, min_scores, eager)
        sb = ra.StreamBatch(ctx, None, cfg, 2, max_chunks_per_call=MAX_CHUNKS, wakewords=[{"model": model, "none_index": none_index}], mfcc_size=K)
        det, _ = feed(sb, pcm, pieces)
        for s in range(2):
            n, _ = check_stream([g[:6] for g in det[s]], lg, L, none_index, cfg)
            assert (n >= 2) if (fires and eager) else n == 0


@pytest.mark.parametrize("avg_threshold,eager,min_scores", [(0.0, False, 1), (R.MOVING_AVG_THRESHOLD, False, 3), (R.MOVING_AVG_THRESHOLD, True, 3)])
def test_live_shared_moving(ra, ctx, device_models, moving_pcm, moving_whole, avg_threshold, eager, min_scores):
    """the moving set through a live batch with the shared model: frame, window, counter and label of the whole-recording run, scores within
    2e-6 (the in-place kernel against the staged-frame kernel)"""
    cfg = config(ra, R.MOVING_THRESHOLD, avg_threshold, min_scores, eager)
    want = moving_whole[(avg_threshold, eager, min_scores)]
    worst = 0.0
    for mi in range(len(R.MOVING)):
        ss = moving_streams(mi)
        sb = ra.StreamBatch(ctx, None, cfg, len(ss), max_chunks_per_call=MAX_CHUNKS, wakewords=[{"model": device_models["moving%d" % mi][1], "none_index": 0}],
                            mfcc_size=K)
        det, _ = feed(sb, moving_pcm[ss], (3, 1, 2))
        for i, s in enumerate(ss):
            assert [g[:3] + (g[5],) for g in det[i]] == [w[:3] + (w[5],) for w in want[s]], (s, det[i], want[s])
            assert len(det[i]) >= (3 if not eager and min_scores == 1 else 1)
            for g, w in zip(det[i], want[s]):
                worst = max(worst, abs(float(g[3]) - float(w[3])), abs(float(g[4]) - float(w[4])))
    print("worst score difference against the whole recording %.3g" % worst)
    assert worst <= 2e-6


# ------------------------------------------------------------------ 6. the single-stream Rustpotter: the host loop
RP_CHUNKS = 20     # 57 frames: two detections of an L = 20 model or more; with the moving streams about five 3 s streams' worth of audio in all


@pytest.mark.parametrize("name", TABLE)
def test_rustpotter_constant(ra, name):
    """a .rpw file holds two layers (Tiny) or three: every vector as a two-layer L = 20 model.  Chunk, counter and name of the reference on
    the bias, scores within 1e-6 of the f64 formula"""
    model = const_model(name, 20, (3,))
    bias, none_index = R.constant_vector(name)
    pcm = R.noise_pcm(1, RP_CHUNKS, seed=3)[0]
    lg = np.tile(bias, (3 * RP_CHUNKS - 3 - 20 + 1, 1))
    fires = name != "nan" and R.CONSTANT[name][2] is not None
    # (this path takes a call per chunk: the avg gate on and eager for every vector, the other two runs for one)
    for avg_threshold, min_scores, eager in ((CONST_AVG, 1, True),) + (((0.0, 3, True), (CONST_AVG, 1, False)) if name == "cab_none0" else ()):
        cfg = config(ra, CONST_THRESHOLD, avg_threshold, min_scores, eager)
        want = R.detect_model_ref(lg, 20, none_index, cfg)
        got = rustpotter_run(ra, model, pcm, cfg)
        assert [(c, r.counter, r.name) for c, r in got] == [(w[0] // 3 + 1, w[2], model["labels"][w[5]]) for w in want], (got, want)
        assert (len(got) >= 2) if (fires and eager) else not got
        if fires:
            f = R.expected_constant(name, avg_threshold)
            assert all(abs(float(r.score) - f[1]) <= 1e-6 and abs(float(r.avg_score) - f[2]) <= 1e-6 for _, r in got)
            assert all(same_bits([r.scores[l] for l in model["labels"]], bias) for _, r in got)


def test_rustpotter_moving(ra, moving_pcm):
    """the moving models in their two-layer form against oracle.rp_oracle.Detector: chunk, counter and name, scores within 1e-5"""
    models = R.moving_models(two_layers=True)
    n = 0
    for s in (0, 1):
        model = models[R.MOVING_STREAM_MODEL[s]]
        cfg = config(ra, R.MOVING_THRESHOLD, R.MOVING_AVG_THRESHOLD, 1, False)
        got = rustpotter_run(ra, model, moving_pcm[s], cfg)
        d = orc.Detector(avg_threshold=cfg.avg_threshold, threshold=cfg.threshold, min_scores=1, eager=False)
        d.add_model(model)
        want = [(i // 480, r) for i in range(0, moving_pcm.shape[1] - 479, 480) for r in [d.process_f32(moving_pcm[s, i:i + 480])] if r is not None]
        assert [(c, r.counter, r.name) for c, r in got] == [(c, r["counter"], r["name"]) for c, r in want], (got, want)
        assert all(abs(float(g.score) - float(w["score"])) <= 1e-5 and abs(float(g.avg_score) - float(w["avg_score"])) <= 1e-5
                   for (_, g), (_, w) in zip(got, want))
        n += len(got)
    assert n >= 6
