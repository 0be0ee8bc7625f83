"""rp_wakeword_model_train_batch / rp_mlp_train_batch: many wakeword models trained in one call (train_batch_kernel: a workgroup per model,
the epochs inside the kernel).  The yardstick of the whole-model tests is the single call, rp_wakeword_model_train: every file, loss and
accuracy of a batch is compared with what that call gives for the same samples, seed and previous model -- bytes with ==, floats bit for
bit.  The epochs alone are compared with the oracle's training loop under the tolerance of test_train_epochs_match_oracle.

The C ABI carries one rp_train_options for the whole call, so fresh models of one call share the model type; models of different types meet
in one call through prev_models (test_model_types_mixed_through_prev_models).  The byte tests therefore run the three heterogeneous sample
sets once per model type."""
import ctypes as C
import json
import os
import struct
import tempfile

import numpy as np
import pytest

import rpw_py
import simstream
from oracle import rp_oracle as orc

pytestmark = pytest.mark.gpu

G = simstream.GOLDEN
EXP = json.load(open(os.path.join(G, "expectations.json")))["train"]
SEEDS = [7, 8, 9]
LR = 0.5


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


def _read(f):
    return open(os.path.join(G, f), "rb").read()


def _models():
    """three sample sets out of the golden one: all six wavs | one wakeword wav dropped | noise0 + two wakeword wavs with a test set
    larger than the train set (Bt > B)"""
    train = [(k, _read(v)) for k, v in EXP["train"].items()]
    test = [(k, _read(v)) for k, v in EXP["test"].items()]
    noise = [t for t in train if "[" not in t[0]]
    word = [t for t in train if "[" in t[0]]
    assert len(noise) == 2 and len(word) == 4
    m0 = (dict(train), dict(test))
    m1 = (dict(noise + word[:3]), dict(test))
    m2 = (dict(noise[:1] + word[:2]), dict(test + [noise[1], word[3]]))
    assert len(m2[1]) > len(m2[0])
    return [m0, m1, m2]


MODELS = _models()
_single_cache = {}


def single(ctx, w, m_type, mfcc_size, epochs, seed, prev=None):
    """the yardstick: rp_wakeword_model_train for model w alone (computed once per argument set)"""
    key = (w, m_type, mfcc_size, epochs, seed, prev)
    if key not in _single_cache:
        _single_cache[key] = ctx.train_wakeword_model(MODELS[w][0], MODELS[w][1], m_type, LR, epochs, 1, mfcc_size, seed=seed, prev_model=prev)
    return _single_cache[key]


def rpw_py_load(data):
    with tempfile.NamedTemporaryFile(suffix=".rpw") as f:
        f.write(data)
        f.flush()
        return rpw_py.load_rpw(f.name)


def bits(v):
    return struct.pack("<f", v)


def same(got, want):
    assert len(got) == len(want)
    for w, (g, s) in enumerate(zip(got, want)):
        assert g[0] == s[0], "model %d: the .rpw bytes differ from the single call's" % w
        assert bits(g[1]) == bits(s[1]), "model %d: loss %r, single call %r" % (w, g[1], s[1])
        assert bits(g[2]) == bits(s[2]), "model %d: accuracy %r, single call %r" % (w, g[2], s[2])


# ---------------------------------------------------------------- 1. the bytes of the single call
@pytest.mark.parametrize("mfcc_size,epochs", [(16, 6), (5, 6), (16, 0)])
@pytest.mark.parametrize("m_type", ["tiny", "small", "medium"])
def test_bytes_of_the_single_call(ctx, m_type, mfcc_size, epochs):
    """three heterogeneous models in one call, seeds 7, 8, 9: each file, loss and accuracy equals the single call's.  mfcc_size 5 gives rows
    whose length is no multiple of 4 (the scalar form of the dot products); epochs 0 is the seeded start and the test forward alone"""
    got = ctx.train_wakeword_models(MODELS, m_type=m_type, learning_rate=LR, epochs=epochs, mfcc_size=mfcc_size, seeds=SEEDS)
    same(got, [single(ctx, w, m_type, mfcc_size, epochs, SEEDS[w]) for w in range(3)])
    if epochs == 0:
        assert all(np.isnan(g[1]) for g in got)


def test_default_seeds_are_the_options_seed_plus_index(ctx):
    """seeds NULL: options->seed + w (the harness passes seed 1)"""
    got = ctx.train_wakeword_models(MODELS[:2], m_type="tiny", learning_rate=LR, epochs=2, mfcc_size=16)
    same(got, [single(ctx, w, "tiny", 16, 2, 1 + w) for w in range(2)])


# ---------------------------------------------------------------- 2. prev_models
def test_prev_models(ctx):
    """model 0 continues from its own 3-epoch result for 3 more epochs, model 1 has a NULL entry in the same call"""
    start = single(ctx, 0, "tiny", 16, 3, 7)[0]
    got = ctx.train_wakeword_models(MODELS[:2], m_type="tiny", learning_rate=LR, epochs=3, mfcc_size=16, seeds=SEEDS[:2], prev_models=[start, None])
    same(got, [single(ctx, 0, "tiny", 16, 3, 7, prev=start), single(ctx, 1, "tiny", 16, 3, 8)])


def test_model_types_mixed_through_prev_models(ctx):
    """Tiny, Small and Medium in ONE call: each model continues a seeded start of its own type (the model's type, mfcc_size and window
    win over the options, as in the single call)"""
    types = ["tiny", "small", "medium"]
    starts = [single(ctx, w, types[w], 16, 0, SEEDS[w])[0] for w in range(3)]
    got = ctx.train_wakeword_models(MODELS, m_type="large", learning_rate=LR, epochs=6, mfcc_size=5, seeds=SEEDS, prev_models=starts)
    same(got, [single(ctx, w, "large", 5, 6, SEEDS[w], prev=starts[w]) for w in range(3)])
    assert [rpw_py_load(g[0])["m_type"] for g in got] == ["Tiny", "Small", "Medium"]


# ---------------------------------------------------------------- 3. the epoch cut changes nothing
@pytest.mark.parametrize("per_launch,launches", [("1", 6), ("4", 2)])
def test_epoch_cut_changes_nothing(ctx, monkeypatch, per_launch, launches):
    """RP_TRAIN_EPOCHS_PER_LAUNCH is read per call; 6 epochs as 6 x 1 and as 4 + 2 give the bytes of the default cut"""
    monkeypatch.delenv("RP_TRAIN_EPOCHS_PER_LAUNCH", raising=False)
    want = ctx.train_wakeword_models(MODELS, m_type="small", learning_rate=LR, epochs=6, mfcc_size=16, seeds=SEEDS)
    assert ctx.train_batch_profile()[2] == 1          # the default bound holds these six epochs in one launch
    monkeypatch.setenv("RP_TRAIN_EPOCHS_PER_LAUNCH", per_launch)
    got = ctx.train_wakeword_models(MODELS, m_type="small", learning_rate=LR, epochs=6, mfcc_size=16, seeds=SEEDS)
    assert ctx.train_batch_profile()[2] == launches
    same(got, want)
    same(got, [single(ctx, w, "small", 16, 6, SEEDS[w]) for w in range(3)])


# ---------------------------------------------------------------- 4. independence of the batch
def candle_linear(rng, dims):
    """candle_nn::linear's initialisation: weights N(0, sqrt(2 / fan_in)), biases U(+-1 / sqrt(fan_in))"""
    return [((rng.standard_normal((dims[l + 1], dims[l])) * np.sqrt(2.0 / dims[l])).astype(np.float32),
             rng.uniform(-1.0, 1.0, dims[l + 1]).astype(np.float32) / np.float32(np.sqrt(dims[l]))) for l in range(len(dims) - 1)]


def random_job(seed, dims, B):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], B).astype(np.int32)
    labels[:min(B, dims[-1])] = np.arange(min(B, dims[-1]))
    return {"dims": list(dims), "x": x, "labels": labels, "params": candle_linear(rng, dims)}


def run_jobs(ctx, jobs, epochs, lr=LR):
    return ctx.mlp_train_batch([j["dims"] for j in jobs], [j["x"] for j in jobs], [j["labels"] for j in jobs], [j["params"] for j in jobs], lr, epochs)


def params_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(wa, wb) and np.array_equal(ba, bb) for (wa, ba), (wb, bb) in zip(a, b))


def test_a_model_does_not_depend_on_its_neighbours(ctx):
    a, b, c = random_job(1, (37, 6, 3), 9), random_job(2, (256, 13, 2), 70), random_job(3, (20, 5), 4)
    p1, l1 = run_jobs(ctx, [a, b, c], 4)
    p2, l2 = run_jobs(ctx, [c, a], 4)
    assert params_equal(p1[0], p2[1]) and params_equal(p1[2], p2[0])
    assert l1[0].tobytes() == l2[1].tobytes() and l1[2].tobytes() == l2[0].tobytes()
    assert not params_equal(p1[0], a["params"])   # and the epochs did something


def test_more_jobs_than_compute_units(ctx):
    """300 copies of one tiny job: the grid walks the jobs, every copy gets the first one's bits"""
    job = random_job(4, (16, 1, 2), 3)
    params, loss = run_jobs(ctx, [job] * 300, 2)
    assert np.isfinite(loss).all()
    for w in range(1, 300):
        assert params_equal(params[w], params[0]), w
    assert all(v.tobytes() == loss[:1].tobytes() for v in np.split(loss, 300))
    one, l_one = run_jobs(ctx, [job], 2)
    assert params_equal(one[0], params[299]) and l_one.tobytes() == loss[:1].tobytes()


# ---------------------------------------------------------------- 5. against the oracle
# (rows, input, hidden widths, labels): rows 65 cross a wave in the loss rows; inputs around 256 put the bias column in + 1 on either side
# of a 256 boundary and 5 / 255 / 257 are no multiples of 4; hidden widths 1 / 3 / 33 are below, no multiple of and above a group of four
# outputs / half a wave; one, two and three layers
ORACLE_CASES = [
    (1, 5, (), 2), (2, 255, (1,), 3), (64, 256, (3,), 5), (65, 257, (33,), 2), (65, 256, (33, 3), 3), (2, 257, (3, 1), 5),
    (1, 255, (33, 33), 2), (64, 5, (1,), 2), (65, 5, (), 5), (2, 256, (), 3), (64, 257, (1, 33), 3), (1, 256, (3,), 2),
]
ORACLE_EPOCHS = 3


@pytest.fixture(scope="module")
def oracle_run(ctx):
    """all the cases as ONE call (a heterogeneous batch), and the oracle's loop per case"""
    jobs = [random_job(100 + i, (n_in,) + hidden + (n_lab,), B) for i, (B, n_in, hidden, n_lab) in enumerate(ORACLE_CASES)]
    got, loss = run_jobs(ctx, jobs, ORACLE_EPOCHS)
    refs = [orc.mlp_train(j["x"], j["labels"], [p[0] for p in j["params"]], [p[1] for p in j["params"]], LR, ORACLE_EPOCHS) for j in jobs]
    return jobs, got, loss, refs


@pytest.mark.parametrize("case", range(len(ORACLE_CASES)), ids=["B%d-in%d-h%s-C%d" % (c[0], c[1], "x".join(map(str, c[2])) or "none", c[3]) for c in ORACLE_CASES])
def test_epochs_match_the_oracle(oracle_run, case):
    """tolerance of test_train_epochs_match_oracle: |loss - ref| <= 1e-4 max(|ref|, 1e-3); per tensor max|got - ref| <= 1e-4 max(max|ref|,
    moved), moved = the largest change the oracle made to that tensor; and the epochs moved some tensor by more than 1e-4"""
    jobs, got, loss, refs = oracle_run
    job, (rw, rb, rloss) = jobs[case], refs[case]
    print("loss %r, oracle %r" % (float(loss[case]), float(rloss)))
    assert abs(float(loss[case]) - rloss) <= 1e-4 * max(abs(rloss), 1e-3)
    moves = []
    for l, (w0, b0) in enumerate(job["params"]):
        for kind, g, ref, start in (("weight", got[case][l][0], rw[l], w0), ("bias", got[case][l][1], rb[l], b0)):
            assert g.shape == ref.shape
            moved = float(np.abs(ref - start).max())
            err = float(np.abs(g - ref).max())
            print("layer %d %s: max error %.3g, moved %.3g" % (l, kind, err, moved))
            assert err <= 1e-4 * max(float(np.abs(ref).max()), moved)
            moves.append(moved)
    assert max(moves) > 1e-4


# ---------------------------------------------------------------- 6. refusals
def raw_call(ctx, models, m_type=0, epochs=1, mfcc_size=16):
    """rp_wakeword_model_train_batch itself: (status, error text, out_rpw pointers, out_lens)"""
    from rustpotter_amd.api import _TrainOptions
    W = len(models)

    def pack(sets):
        names = [k.encode() for d in sets for k in d]
        bufs = [bytes(v) for d in sets for v in d.values()]
        n = len(names)
        return (C.c_size_t * W)(*[len(d) for d in sets]), (C.c_char_p * n)(*names), (C.c_char_p * n)(*bufs), (C.c_size_t * n)(*[len(b) for b in bufs])
    tr, te = pack([m[0] for m in models]), pack([m[1] for m in models])
    opt = _TrainOptions(m_type, LR, epochs, 0, mfcc_size, 1)
    out, out_lens = (C.c_void_p * max(W, 1))(), (C.c_size_t * max(W, 1))()
    for w in range(W):
        out[w], out_lens[w] = 0xdead0, 77   # the call must clear what it does not fill
    r = ctx._L.rp_wakeword_model_train_batch(ctx._h, C.byref(opt), W, None, *tr, *te, None, None, out, out_lens, None, None)
    return r, ctx._L.rp_last_error().decode(), [out[w] for w in range(W)], [out_lens[w] for w in range(W)]


def test_refusals_name_the_model_and_leave_every_output_null(ctx):
    m0, m1, m2 = MODELS
    only_noise = ({k: v for k, v in m0[0].items() if "[" not in k}, {k: v for k, v in m0[1].items() if "[" not in k})
    alexa = (m2[0], dict(m2[1], **{"x[Alexa].wav": _read("alexa.wav")}))
    for models, text in (([m0, ({}, m1[1]), m2], "model 1: No training data provided"),
                         ([only_noise, m1], "model 0: Your training data need to contain at least two labels"),
                         ([m0, m1, alexa], "model 2: Forbidden label 'alexa'")):
        r, err, out, lens = raw_call(ctx, models)
        assert r == -1 and err.startswith(text), err
        assert all(p is None for p in out) and all(n == 0 for n in lens)
    with pytest.raises(Exception, match="model 1: No training data provided"):
        ctx.train_wakeword_models([m0, ({}, m1[1])], m_type="tiny", epochs=1)


def test_no_models_is_a_success(ctx):
    r, _, _, _ = raw_call(ctx, [])
    assert r == 0
    assert ctx.train_wakeword_models([], m_type="tiny") == []
    params, loss = ctx.mlp_train_batch([], [], [], [], LR, 3)
    assert params == [] and loss.shape == (0,)


def test_mlp_train_batch_refuses_by_model(ctx, ra):
    job, bad = random_job(5, (8, 2), 3), random_job(6, (8, 2), 3)
    bad["labels"][1] = 2
    before = [(w.copy(), b.copy()) for w, b in job["params"]]
    with pytest.raises(ra.RustpotterError, match="model 1: label out of range"):
        run_jobs(ctx, [job, bad], 2)
    assert params_equal(job["params"], before)
    _, loss = run_jobs(ctx, [job], 0)
    assert np.isnan(loss).all()   # no epoch, no loss


# ---------------------------------------------------------------- 7. into a bank
def test_models_of_a_batch_go_into_a_model_bank(ra, ctx):
    got = ctx.train_wakeword_models(MODELS, m_type="tiny", learning_rate=LR, epochs=6, mfcc_size=16, seeds=SEEDS)
    files = [rpw_py_load(g[0]) for g in got]
    bank = ctx.model_bank(rpw=[g[0] for g in got])
    assert bank.W == 3
    assert bank.train_sizes == [f["train_size"] for f in files]
    assert bank.labels == [len(f["labels"]) for f in files]
    pcm = np.zeros((2, 16000 * 3), np.float32)
    det, dlab, n_det = ctx.batch_detect_model_bank(pcm, bank, np.array([0, 2], np.int32), ra.DetectorConfig())
    assert not n_det.any()
