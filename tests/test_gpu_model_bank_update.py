"""A model bank that changes: rp_model_bank_reserve / _put / _put_from_rpw / _train / _read_image (model_bank_put_kernel builds a model's
bank image on the device from its raw parameters, model_bank_move_kernel carries the live models of a full pool into a larger one), also
under live-stream batches.  Every comparison is BIT FOR BIT against a route that was there before: a bank made in one go by rp_model_bank_new
(Model::create's host-side image), rp_wakeword_model_train_batch followed by rp_model_bank_new_from_rpw, an undisturbed live batch.  No
tolerance is involved anywhere.
The six models, their shapes and the synthetic MFCC rows are those of tests/test_gpu_model_bank.py; the live set-up (detection weights,
threshold, feed) is that of tests/test_gpu_stream_model_bank.py; the training sets are the first two of tests/test_gpu_train_batch.py."""
import os
import struct

import numpy as np
import pytest

import rpw_py
from test_gpu_model_bank import DET_GAIN, DET_MODEL_SEED, DET_SEED, K, MODELS, NONE_INDEX, STREAM_MODEL, S, bank_weights, model_dict, synth_mfcc
from test_gpu_stream_model_bank import MAX_CHUNKS, config, feed
from test_gpu_train_batch import G, LR, _models

pytestmark = pytest.mark.gpu
TRAIN_SETS = _models()[0:2]
TRAIN_SEEDS = [7, 8]
CHUNKS = 100   # 3 s: the longest window (256 frames) lies inside the audio for the last 40 frames


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
    """the yardstick: all six in one go"""
    return ra.ModelBank(ctx, models=models, none_index=NONE_INDEX)


@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(430)
    return {nf: synth_mfcc(rng, S, nf) for nf in (430, 220)}


def rpw_of(i, ws, bs):
    return rpw_py.dump_rpw_model(**model_dict(i, ws, bs))


def images(b):
    return [b.read_image(w) for w in range(b.W)]


def state(b):
    """everything a refused call must leave as it was"""
    return (b.W, list(b.train_sizes), list(b.labels), b.max_train_size, b.label_pitch, b.reserved, images(b))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_banks(ctx, got, want, rows, idx):
    assert (got.W, got.train_sizes, got.labels, got.max_train_size) == (want.W, want.train_sizes, want.labels, want.max_train_size)
    gi, wi = images(got), images(want)
    for w in range(want.W):
        assert len(gi[w]) == len(wi[w]) > want.train_sizes[w] * 192 * 16
        assert gi[w] == wi[w], "model %d: %d image bytes differ" % (w, sum(x != y for x, y in zip(gi[w], wi[w])))
    for nf, mfcc in rows.items():
        a, b = ctx.mlp_forward_windows_bank(mfcc, got, idx), ctx.mlp_forward_windows_bank(mfcc, want, idx)
        n = min(a.shape[2], b.shape[2])
        assert same_bits(np.ascontiguousarray(a[:, :, :n]), np.ascontiguousarray(b[:, :, :n])), nf
        assert not a[:, :, n:].any() and not b[:, :, n:].any()


# ---------------------------------------------------------------- 1. put equals create
@pytest.mark.parametrize("route", ["put", "put_rpw"])
def test_put_equals_create(ra, ctx, weights, models, bank, rows, route):
    """an empty bank, two puts of three models each: the images, the logits of the 430-frame and the 220-frame rows and the accessors are
    those of the bank made in one go"""
    b = ra.ModelBank(ctx, models=[])
    assert b.W == 0 and b.label_pitch == 0 and b.max_train_size == 0 and b.pool_growths == 0
    b.put(0, [])   # n == 0 succeeds and changes nothing
    assert b.W == 0
    for first in (0, 3):
        if route == "put":
            b.put(first, models[first:first + 3], NONE_INDEX[first:first + 3])
        else:
            b.put_rpw(first, [rpw_of(i, *weights[i]) for i in range(first, first + 3)])
        assert b.W == first + 3
    assert b.label_pitch == bank.label_pitch and b.reserved == (0, 0) and b.pool_growths >= 1
    same_banks(ctx, b, bank, rows, STREAM_MODEL)


# ---------------------------------------------------------------- 2. special parameters
F32_MAX = np.float32(3.4028234663852886e38)
SPECIALS = np.array([0.0, -0.0, 1.401298464324817e-45, -1.401298464324817e-45, 2.0 ** -126, -2.0 ** -126, 1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23),
                     F32_MAX, -F32_MAX,
                     # the second leftover of the three-part split is subnormal (the truncation fallback cuts it)
                     2.0 ** -118 * (1 + 2.0 ** -7 + 2.0 ** -15 + 2.0 ** -22), -2.0 ** -120 * (1 + 2.0 ** -8 + 2.0 ** -16 + 2.0 ** -23),
                     2.0 ** -112 * (1 + 2.0 ** -8 + 2.0 ** -17 + 2.0 ** -23), 2.0 ** -125 * (1 + 2.0 ** -3 + 2.0 ** -11),
                     # the first part rounds up into the next binade; a tie; the largest subnormal
                     1.99999988, 1.00390625, 1.1754942106924411e-38, 3.3895313892515355e38, 65504.0, -3.0e-39], np.float32)


def special_model(L, d1, seed):
    """a Tiny model [16 L, d1, 2] whose layer 1 cycles through SPECIALS between random values"""
    rng = np.random.default_rng(seed)
    w1 = (rng.standard_normal((d1, 16 * L)) / 4).astype(np.float32)
    flat = w1.reshape(-1)
    at = rng.permutation(flat.size)[:max(flat.size // 2, min(flat.size, len(SPECIALS)))]
    flat[at] = SPECIALS[np.arange(at.size) % len(SPECIALS)]
    b1 = (rng.standard_normal(d1) * 0.1).astype(np.float32)
    b1[::3] = SPECIALS[np.arange(len(b1[::3])) % 8]
    w2 = (rng.standard_normal((2, d1)) / np.sqrt(d1)).astype(np.float32)
    w2[0, 0] = np.float32(-0.0)
    b2 = np.array([1.401298464324817e-45, -0.25], np.float32)
    return [w1, w2], [b1, b2]


@pytest.mark.parametrize("d1", [1, 16, 17, 32])
@pytest.mark.parametrize("L", [1, 3])
def test_special_parameters(ra, ctx, L, d1):
    """zeros of both signs, subnormals, the smallest normal, 1 + ulp, +-FLT_MAX (rounds to bf16 infinity: the truncation fallback) and
    values with a subnormal second leftover, in both widths of b1 / wsum (16, 32 rows) and a full tile: image bytes against
    rp_model_bank_new, through the handle route and the .rpw route"""
    ws, bs = special_model(L, d1, 100 * L + d1)
    assert np.isin(SPECIALS[:min(len(SPECIALS), ws[0].size)].view(np.uint32), ws[0].view(np.uint32)).all()
    m = ra.Model(ctx, ws, bs)
    want = ra.ModelBank(ctx, models=[m], none_index=[0]).read_image(0)
    assert len(want) == L * 192 * 16 + (16 if d1 <= 16 else 32) * 17 * 4 + ((2 * d1 + 2 + 3) & ~3) * 4
    md = {"labels": ["none", "a"], "train_size": L, "mfcc_size": K, "m_type": "tiny", "rms_level": float("nan"),
          "weights": {"ln1.weight": ws[0], "ln1.bias": bs[0], "ln2.weight": ws[1], "ln2.bias": bs[1]}}
    b = ra.ModelBank(ctx, models=[])
    b.put(0, [m], [0])
    b.put_rpw(1, [rpw_py.dump_rpw_model(**md)])
    for w in range(2):
        got = b.read_image(w)
        assert len(got) == len(want)
        assert got == want, "route %d: %d image bytes differ, first at %d" % (w, sum(x != y for x, y in zip(got, want)), next(i for i in range(len(want)) if got[i] != want[i]))


@pytest.mark.parametrize("where,value", [("ln1.weight", np.inf), ("ln1.weight", np.nan), ("ln1.bias", -np.inf), ("ln2.weight", np.nan), ("ln2.bias", np.inf)])
def test_non_finite_parameters_are_refused(ra, ctx, weights, models, where, value):
    b = ra.ModelBank(ctx, models=models[:2], none_index=NONE_INDEX[:2])
    before = state(b)
    md = model_dict(0, *weights[0])
    md["weights"] = {k: v.copy() for k, v in md["weights"].items()}
    md["weights"][where].reshape(-1)[-1] = value
    with pytest.raises(ra.RustpotterError, match="wakeword 2: parameters must be finite"):
        b.put_rpw(1, [rpw_of(1, *weights[1]), rpw_py.dump_rpw_model(**md)])
    assert state(b) == before


# ---------------------------------------------------------------- 3. replace and growth
def test_replace_and_growth(ra, ctx, models, rows):
    """a bank whose pools start exactly full grows put by put, with two indices replaced by models of other shapes on the way (their old
    entries are garbage the next growth drops): afterwards it is the bank made in one go from the final list"""
    cur = [0, 1]
    b = ra.ModelBank(ctx, models=[models[i] for i in cur], none_index=[NONE_INDEX[i] for i in cur])
    assert b.pool_growths == 0
    growths = []
    for first, ids in ((2, [2]), (0, [4]), (3, [3, 5]), (1, [0]), (5, [1, 2]), (2, [5, 3])):
        b.put(first, [models[i] for i in ids], [NONE_INDEX[i] for i in ids])
        cur[first:first + len(ids)] = ids
        growths.append(b.pool_growths)
        assert b.W == len(cur) and b.train_sizes == [MODELS[i][1] for i in cur]
    print("pool growths after each put:", growths)
    assert growths[0] >= 1 and growths[-1] > growths[1] >= 2   # a growth after each replacement
    want = ra.ModelBank(ctx, models=[models[i] for i in cur], none_index=[NONE_INDEX[i] for i in cur])
    same_banks(ctx, b, want, rows, np.array([k % len(cur) if k != 3 else -1 for k in range(S)], np.int32))


# ---------------------------------------------------------------- 4. train equals train + load
def fbits(v):
    return struct.pack("<f", v)


@pytest.fixture(scope="module")
def golden_pcm():
    """the 16 kHz mono i16 recordings of the golden training set, zero padded to one length"""
    recs = []
    for f in sorted(os.listdir(G)):
        if f.endswith(".wav") and (f.startswith("oye_casa") or f.startswith("noise")):
            a, sr, ch = rpw_py.read_wav(os.path.join(G, f))
            if sr == 16000 and ch == 1 and a.dtype == np.dtype("<i2"):
                recs.append(a)
    assert len(recs) >= 4
    recs = recs[:12]
    n = (max(len(a) for a in recs) + 16000 + 479) // 480 * 480
    pcm = np.zeros((len(recs), n), np.int16)
    for s, a in enumerate(recs):
        pcm[s, 8000:8000 + len(a)] = a
    return pcm


@pytest.mark.parametrize("case", ["files", "no_files", "prev"])
def test_train_equals_train_and_load(ra, ctx, golden_pcm, case):
    """rp_model_bank_train into a reserved empty bank against rp_wakeword_model_train_batch -> rp_model_bank_new_from_rpw: files, loss and
    accuracy, image bytes, and the detections of both banks over the golden recordings"""
    prev, epochs = None, 6
    if case == "prev":
        start = ctx.train_wakeword_models(TRAIN_SETS, m_type="tiny", learning_rate=LR, epochs=3, mfcc_size=16, seeds=TRAIN_SEEDS)
        prev, epochs = [start[0][0], None], 3
    want = ctx.train_wakeword_models(TRAIN_SETS, m_type="tiny", learning_rate=LR, epochs=epochs, mfcc_size=16, seeds=TRAIN_SEEDS, prev_models=prev)
    wbank = ctx.model_bank(rpw=[g[0] for g in want])
    b = ra.ModelBank(ctx, models=[])
    b.reserve(256, 3)
    assert b.reserved == (256, 3) and b.label_pitch == 3 and b.W == 0
    got = b.train(0, TRAIN_SETS, m_type="tiny", learning_rate=LR, epochs=epochs, seeds=TRAIN_SEEDS, prev_models=prev, want_rpw=case != "no_files")
    for w in range(2):
        assert got[w][0] == (None if case == "no_files" else want[w][0]), w
        assert fbits(got[w][1]) == fbits(want[w][1]) and fbits(got[w][2]) == fbits(want[w][2]), (w, got[w][1:], want[w][1:])
    assert (b.W, b.train_sizes, b.labels) == (2, wbank.train_sizes, wbank.labels)
    assert images(b) == images(wbank)
    cfg = ra.DetectorConfig()
    cfg.threshold, cfg.avg_threshold, cfg.min_scores = 0.0, 0.0, 1   # every window whose label is not "none" counts: six epochs decide little
    idx = np.arange(golden_pcm.shape[0], dtype=np.int32) % 2
    d1, l1, n1 = ctx.batch_detect_model_bank(golden_pcm, b, idx, cfg)
    d2, l2, n2 = ctx.batch_detect_model_bank(golden_pcm, wbank, idx, cfg)
    print(case, "detections per recording:", n1.tolist())
    assert np.array_equal(n1, n2) and d1.tobytes() == d2.tobytes() and np.array_equal(l1, l2)
    # what the scores are made of (six epochs may leave every window at "none"): the logits of every window of the recordings
    mf = ctx.mfcc(golden_pcm.astype(np.float32) / np.float32(32768), 16)
    a, w = ctx.mlp_forward_windows_bank(mf, b, idx), ctx.mlp_forward_windows_bank(mf, wbank, idx)
    assert a.shape[2] == 3 and w.shape[2] == 2 and a[:, :, :2].any() and not a[:, :, 2].any()
    assert same_bits(np.ascontiguousarray(a[:, :, :2]), w)


# ---------------------------------------------------------------- 5. live growth
@pytest.fixture(scope="module")
def det_weights():
    return bank_weights(DET_MODEL_SEED, DET_GAIN)


@pytest.fixture(scope="module")
def det_models(ra, ctx, det_weights):
    return [ra.Model(ctx, ws, bs) for ws, bs in det_weights]


@pytest.fixture(scope="module")
def live_pcm(ctx):
    return ctx.synth_pcm(DET_SEED, 0, 6, 480 * CHUNKS)


def live_batch(ra, ctx, b, idx):
    return ra.StreamBatch(ctx, None, config(ra), len(idx), max_chunks_per_call=MAX_CHUNKS, model_bank=b, stream_model=np.asarray(idx, np.int32))


def test_live_growth(ra, ctx, det_models, live_pcm):
    """six streams over a reserved empty bank; models arrive while the batch runs (the later puts replace the pools) and their streams are
    connected.  Every stream carries the logits and detections of the same schedule over a bank that held all six from the start."""
    b = ra.ModelBank(ctx, models=[])
    b.reserve(256, 3)
    whole = ra.ModelBank(ctx, models=det_models, none_index=NONE_INDEX)
    assert whole.label_pitch == 3 == b.label_pitch
    sb, sw = live_batch(ra, ctx, b, [-1] * 6), live_batch(ra, ctx, whole, [-1] * 6)
    growths = {}
    connect = {9: (0, [0, 1, 2]), 30: (3, [3, 4]), 45: (5, [5])}

    def arrive(c):
        if c in connect:
            first, ids = connect[c]
            b.put(first, [det_models[i] for i in ids], [NONE_INDEX[i] for i in ids])
            growths[c] = b.pool_growths
            sb.set_models(first, np.array(ids, np.int32))

    def connect_only(c):
        if c in connect:
            sw.set_models(connect[c][0], np.array(connect[c][1], np.int32))
    det, lg = feed(sb, live_pcm, (3,), before_chunk=arrive)
    wdet, wlg = feed(sw, live_pcm, (3,), before_chunk=connect_only)
    print("pool growths at the puts:", growths, "detections per stream:", [len(d) for d in det])
    assert growths[9] >= 1 and growths[30] > growths[9] and growths[45] > growths[30]   # streams 0-2 ran through two pool replacements
    assert b.W == 6 and not lg[:, :27].any()
    for c, (first, ids) in connect.items():
        for s, mi in zip(range(first, first + len(ids)), ids):
            assert not lg[s, :3 * c].any(), s
            at = max(3 * c, MODELS[mi][1] + 2)   # from its connection on, the windows that lie inside the audio
            assert same_bits(np.ascontiguousarray(lg[s, at:]), np.ascontiguousarray(wlg[s, at:])) and lg[s, at:].any(), (s, mi)
    assert det == wdet
    sb.close()
    sw.close()


def test_live_replacement(ra, ctx, det_models, live_pcm):
    """a stream whose index is replaced between calls gives the new model's logits from the next call on: on full windows those of a batch
    over the new model fed the same audio.  Its neighbours never notice."""
    b = ra.ModelBank(ctx, models=[])
    b.reserve(256, 3)
    b.put(0, [det_models[0], det_models[1]], NONE_INDEX[:2])
    new = ra.ModelBank(ctx, models=[det_models[2], det_models[1]], none_index=[NONE_INDEX[2], NONE_INDEX[1]])
    old = ra.ModelBank(ctx, models=det_models[:2], none_index=NONE_INDEX[:2])
    idx = [0, 1, 0, -1, 1, 0]
    sb = live_batch(ra, ctx, b, idx)

    def replace(c):
        if c == 30:
            b.put(0, [det_models[2]], [NONE_INDEX[2]])   # L 30 -> 75, 2 labels -> 3
    _, lg = feed(sb, live_pcm, (3,), before_chunk=replace)
    _, lg_new = feed(live_batch(ra, ctx, new, idx), live_pcm, (3,))
    _, lg_old = feed(live_batch(ra, ctx, old, idx), live_pcm, (3,))
    assert lg.shape[2] == 3 and lg_new.shape[2] == 3 and lg_old.shape[2] == 2
    at = 3 * 30   # the first column of the call that follows the put; the window of 75 frames that ends there lies inside the audio
    for s, mi in enumerate(idx):
        if mi == 0:
            assert same_bits(np.ascontiguousarray(lg[s, at:]), np.ascontiguousarray(lg_new[s, at:])), s
            assert same_bits(np.ascontiguousarray(lg[s, 32:at, :2]), np.ascontiguousarray(lg_old[s, 32:at])) and not lg[s, :at, 2].any(), s
            assert not np.array_equal(lg[s, at:, :2], lg_old[s, at:])
        elif mi == 1:
            assert same_bits(np.ascontiguousarray(lg[s, 197:]), np.ascontiguousarray(lg_new[s, 197:])) and lg[s, 197:].any(), s
        else:
            assert not lg[s].any()
    sb.close()


# ---------------------------------------------------------------- 6. reservation changes no bits
def test_reservation_changes_no_bits(ra, ctx, det_models, live_pcm):
    ids = [0, 1, 2, 3, 5]   # the longest window is 195 frames: room for a larger reservation
    plain = ra.ModelBank(ctx, models=[det_models[i] for i in ids], none_index=[NONE_INDEX[i] for i in ids])
    res = ra.ModelBank(ctx, models=[det_models[i] for i in ids], none_index=[NONE_INDEX[i] for i in ids])
    res.reserve(256, 5, 16, 2000)
    assert (plain.label_pitch, res.label_pitch) == (3, 5) and res.max_train_size == plain.max_train_size == 195
    assert images(res) == images(plain)
    idx = [4, 0, 3, 1, 2, -1]
    d1, lg1 = feed(live_batch(ra, ctx, plain, idx), live_pcm, (4,))
    d2, lg2 = feed(live_batch(ra, ctx, res, idx), live_pcm, (4,))
    assert lg1.shape[2] == 3 and lg2.shape[2] == 5
    assert not lg2[:, :, 3:].any()
    for s, w in enumerate(idx):
        at = MODELS[ids[w]][1] + 2 if w >= 0 else 0   # the windows that lie inside the audio
        nl = len(MODELS[ids[w]][3]) if w >= 0 else 0
        assert same_bits(np.ascontiguousarray(lg1[s, at:]), np.ascontiguousarray(lg2[s, at:, :3])) and not lg1[s, :, nl:].any(), s
    print("detections per stream:", [len(d) for d in d1])
    assert d1 == d2


# ---------------------------------------------------------------- 7. refusals leave the bank as it was
def tiny(ra, ctx, L, d1, labels, seed=3, context=None):
    rng = np.random.default_rng(seed)
    dims = [16 * L, d1, labels]
    ws = [(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32) for i in range(2)]
    bs = [(rng.standard_normal(dims[i + 1]) * 0.1).astype(np.float32) for i in range(2)]
    return ra.Model(context or ctx, ws, bs), ws, bs


def tiny_rpw(L, ws, bs, mfcc_size=K):
    return rpw_py.dump_rpw_model(["none"] + ["l%d" % i for i in range(1, ws[1].shape[0])], L, mfcc_size, "tiny",
                                 {"ln1.weight": ws[0], "ln1.bias": bs[0], "ln2.weight": ws[1], "ln2.bias": bs[1]})


def test_refusals_leave_the_bank_as_it_was(ra, ctx, weights, models):
    b = ra.ModelBank(ctx, models=models[:2], none_index=NONE_INDEX[:2])
    before = state(b)

    def refused(text, call):
        with pytest.raises(ra.RustpotterError, match=text):
            call()
        assert state(b) == before, text
    refused("first model index 3 is past the bank's 2 models", lambda: b.put(3, [models[2]]))
    refused("first model index 3 is past the bank's 2 models", lambda: b.put_rpw(3, [rpw_of(2, *weights[2])]))
    long_m, lw, lb = tiny(ra, ctx, 257, 2, 2)
    refused("model 2: a window of 257 frames; the model bank takes windows of at most 256 frames", lambda: b.put(1, [models[2], long_m]))
    refused("wakeword 1: a window of 257 frames; the model bank takes windows of at most 256 frames", lambda: b.put_rpw(1, [tiny_rpw(257, lw, lb)]))
    wide_m, ww_, wb_ = tiny(ra, ctx, 30, 33, 2)
    refused("model 2: layer 1 is 33 wide; the model bank takes layer 1 at most 32 wide", lambda: b.put(2, [wide_m]))
    refused("wakeword 0: layer 1 is 33 wide", lambda: b.put_rpw(0, [tiny_rpw(30, ww_, wb_)]))
    ref = open(os.path.join(G, "oye_casa_g.rpw"), "rb").read()
    refused("wakeword 3: a wakeword reference cannot be part of a model bank", lambda: b.put_rpw(2, [rpw_of(2, *weights[2]), ref]))
    _, w5, b5 = tiny(ra, ctx, 96, 2, 2)   # 96 * 5 = 30 * 16 features
    refused("model bank: mfcc_size 5 is not built", lambda: b.put_rpw(2, [tiny_rpw(96, w5, b5, mfcc_size=5)]))
    refused("wakeword 3: Usage of wakewords with different mfcc size is not supported", lambda: b.put_rpw(2, [rpw_of(2, *weights[2]), tiny_rpw(96, w5, b5, mfcc_size=5)]))
    other = ra.BatchContext(device=0, host_pointers=True)
    foreign, _, _ = tiny(ra, ctx, 30, 2, 2, context=other)
    refused("model 2: the model belongs to another context", lambda: b.put(2, [foreign]))
    refused("model 2: none_index out of range", lambda: b.put(2, [models[2]], [3]))
    refused("max_train_size 100 is below the bank's longest window", lambda: b.reserve(100, 0))
    refused("max_train_size 257", lambda: b.reserve(257, 0))
    refused("max_labels 33", lambda: b.reserve(0, 33))
    # with a reservation: what exceeds it
    b.reserve(200, 2)
    before = state(b)
    assert before[5] == (200, 2) and before[4] == 2
    refused("model 2: a window of 256 frames is longer than the bank's reserved train size \\(200 frames, rp_model_bank_reserve\\)", lambda: b.put(2, [models[4]]))
    refused("wakeword 0: 3 labels are more than the bank's reserved label count \\(2, rp_model_bank_reserve\\)", lambda: b.put_rpw(0, [rpw_of(2, *weights[2])]))
    # a training the single call refuses, and what the bank does not take
    m0, m1 = TRAIN_SETS
    refused("model 3: No training data provided", lambda: b.train(2, [m0, ({}, m1[1])], epochs=1))
    refused("model bank: mfcc_size 5 is not built", lambda: b.train(2, [m0], epochs=1, mfcc_size=5))
    refused("first model index 3 is past", lambda: b.train(3, [m0], epochs=1))
    refused("model 2: layer 1 is 56 wide", lambda: b.train(2, [m0], m_type="medium", epochs=1))


def test_refusals_under_a_live_batch(ra, ctx, models):
    """without a reservation, while a batch exists: nothing longer or with more labels than the bank holds, and no new reservation"""
    b = ra.ModelBank(ctx, models=models[:1], none_index=NONE_INDEX[:1])   # a window of 30 frames, 2 labels
    sb = live_batch(ra, ctx, b, [0, -1])
    before = state(b)

    def refused(text, call):
        with pytest.raises(ra.RustpotterError, match=text):
            call()
        assert state(b) == before, text
    refused("model 1: a window of 195 frames is longer than the bank's longest \\(30 frames\\) while a stream batch runs over the bank: call rp_model_bank_reserve before creating the batch",
            lambda: b.put(1, [models[1]]))
    three, _, _ = tiny(ra, ctx, 30, 2, 3)
    refused("model 0: 3 labels are more than the bank's largest label count \\(2\\) while a stream batch runs over the bank: call rp_model_bank_reserve before creating the batch",
            lambda: b.put(0, [three]))
    refused("rp_model_bank_reserve: the reserved train size and label count can only change while no stream batch runs over the bank", lambda: b.reserve(256, 0))
    refused("rp_model_bank_reserve: the reserved train size and label count can only change", lambda: b.reserve(0, 3))
    b.reserve(0, 0, 8, 400)   # pool hints alone are no change of the reservation
    assert state(b) == before and b.pool_growths == 1
    short, _, _ = tiny(ra, ctx, 20, 3, 2)
    b.put(1, [short], [0])    # what fits goes in under the batch
    assert b.W == 2 and b.train_sizes == [30, 20]
    sb.close()
    b.reserve(256, 3)         # the batch is gone
    b.put(2, [models[1], three])
    assert b.W == 4 and b.reserved == (256, 3) and b.label_pitch == 3
