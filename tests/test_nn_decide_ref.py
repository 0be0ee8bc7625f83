"""Pins tests/nn_decide_ref.py -- the decision stage of a wakeword model restated from the Rust source, which tests/test_gpu_nn_decide.py
holds the kernels and the host loop against -- to the oracle's chunk-by-chunk detector (oracle.rp_oracle.Detector.add_model, 480-sample
chunks) on the steered inputs of that file: equal chunk, counter and label name, scores within 1e-5, the project's bar against the oracle.

It also asserts, on the reference alone, what the GPU tests rely on: the constant models decide as their table says, and the moving set
has enough detections, counters above 1, detections whose best window carries another label than their first or last window, and no
window near a gate.  No GPU is needed."""
import numpy as np
import pytest

import nn_decide_ref as R
from oracle import rp_oracle as orc

F32 = np.float32
CONST_THRESHOLD = 0.2          # below 0.2689 = 1 - 1 / (1 + e^-1), the score of a window whose label and none logits are equal
CONST_CHUNKS = 40              # 117 frames: several detections of an L = 40 model in eager mode


def oracle_run(model, pcm, cfg):
    """-> [(chunk, result)] of orc.Detector with that one model over 480-sample chunks"""
    d = orc.Detector(avg_threshold=cfg.avg_threshold, threshold=cfg.threshold, min_scores=cfg.min_scores, eager=cfg.eager, score_ref=cfg.score_ref)
    d.add_model(model)
    return [(i // 480, r) for i in range(0, len(pcm) - 479, 480) for r in [d.process_f32(pcm[i:i + 480])] if r is not None]


def same_as_oracle(got, want, labels):
    """detect_model_ref's detections against the oracle's: the chunk that returns it, counter and label name exact, scores within 1e-5"""
    assert len(got) == len(want), (got, want)
    worst = 0.0
    for (frame, window, counter, avg_score, score, label), (chunk, r) in zip(got, want):
        assert frame // 3 + 1 == chunk and counter == r["counter"] and labels[label] == r["name"], (frame, counter, label, chunk, r)
        worst = max(worst, abs(float(score) - float(r["score"])), abs(float(avg_score) - float(r["avg_score"])))
    assert worst <= 1e-5, worst
    return worst


def oracle_logits(model, pcm):
    mf = orc.mfcc_stream(pcm, R.K)
    L = model["train_size"]
    win = np.stack([orc.normalize(mf[w:w + L]).reshape(-1) for w in range(mf.shape[0] - L + 1)])
    return orc.mlp_forward(win, model["ws"], model["bs"])


def test_total_cmp_key_orders_like_f32_total_cmp():
    neg_nan = np.array([0xFFC00000], np.uint32).view(F32)[0]
    order = [neg_nan, F32(-np.inf), F32(-1), F32(-1e-45), F32(-0.0), F32(0.0), F32(1e-45), F32(1), F32(np.inf), F32(np.nan)]
    keys = [R.total_cmp_key(v) for v in order]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert R.get_label([F32(0.0), F32(-0.0)]) == 0 and R.get_label([F32(-0.0), F32(0.0)]) == 1      # -0 < +0
    assert R.get_label([F32(1), F32(1), F32(0)]) == 1                                                # the last of equal maxima
    assert R.get_label([F32(np.nan), F32(np.inf)]) == 0 and R.get_label([neg_nan, F32(-np.inf)]) == 1


@pytest.mark.parametrize("avg_threshold", [0.0, 0.2])
@pytest.mark.parametrize("name", list(R.CONSTANT))
def test_constant_vectors_decide_as_the_table_says(name, avg_threshold):
    bias, none_index, _ = R.CONSTANT[name]
    assert np.all(np.abs(bias) < 4)
    want = R.expected_constant(name, avg_threshold)
    got = R.decide(bias, none_index, 0.22, CONST_THRESHOLD, avg_threshold)
    if want is None:
        assert got is None
        # not for want of a score: with every gate open it is still the none label
        assert R.decide(bias, none_index, 0.22, -1.0, 0.0) is None
        return
    assert got is not None and got[0] == want[0], (got, want)
    assert abs(float(got[1]) - want[1]) <= 1e-6 and abs(float(got[2]) - want[2]) <= 1e-6, (got, want)
    f64 = R.decide_f64(bias, none_index, 0.22, avg_threshold)
    assert f64[0] == want[0] and abs(f64[1] - want[1]) <= 1e-12 and abs(f64[2] - want[2]) <= 1e-12
    # every window passes both gates with room: the table's runs never depend on a rounding
    assert want[1] - CONST_THRESHOLD > 1e-2 and (avg_threshold == 0.0 or want[2] - avg_threshold > 1e-2)


def test_table_values():
    """the figures the issue's table names, spelled out"""
    f = R._f
    a, b, c = float(R.A), float(R.B), float(R.C)
    assert a > b > c
    assert R.expected_constant("aa_none0", 0.2) == (1, f(0.0), f(a))          # nothing left: second 0
    assert abs(f(0.0) - (1 - 1 / (1 + np.exp(-1.0)))) < 1e-7                    # 0.2689 (10 * 0.22 in f32 is not 2.2 in f64)
    assert R.expected_constant("aa_nonone", 0.2) == (1, f(a), f(a))
    assert R.expected_constant("baa_none0", 0.2) == (2, f(a - b), f(a - b))
    assert R.expected_constant("abc_none2", 0.2) == (0, f(a - c), f(a - c))    # second is c, the smallest; not b
    assert R.expected_constant("cab_none0", 0.2) == (1, f(a - c), f(a - c))
    assert R.expected_constant("a_nonone", 0.2) == (0, f(a), f(a))
    wide = R.CONSTANT["wide32_none0"][0]
    assert wide.shape == (32,) and wide[7] == wide[31] == R.A and np.sum(wide == R.A) == 2
    assert R.expected_constant("wide32_none0", 0.2) == (31, f(a - float(wide[0])), f(a - float(wide.min())))


@pytest.mark.parametrize("hidden", [(), (3,)])
@pytest.mark.parametrize("name", list(R.CONSTANT))
def test_constant_models_against_the_oracle(name, hidden):
    """the bias repeated for every window through detect_model_ref equals the oracle's detector on a model that answers it: eager with
    min_scores 1 and 3, both avg thresholds; not eager, every window passes and the countdown never runs out: nothing is reported"""
    bias, none_index, want = R.CONSTANT[name]
    L = 20 if len(bias) % 2 else 40
    model = R.constant_model(bias, none_index, L, hidden)
    pcm = R.noise_pcm(1, CONST_CHUNKS)[0]
    lg = oracle_logits(model, pcm)
    assert lg.shape == (3 * CONST_CHUNKS - 3 - L + 1, len(bias))
    assert np.array_equal(lg.view(np.uint32), np.tile(bias, (len(lg), 1)).view(np.uint32))
    n = 0
    for avg_threshold in (0.0, 0.2):
        for eager, min_scores in ((True, 1), (True, 3), (False, 1)):
            cfg = R.Cfg(CONST_THRESHOLD, avg_threshold, min_scores, eager)
            got = R.detect_model_ref(lg, L, none_index, cfg)
            same_as_oracle(got, oracle_run(model, pcm, cfg), model["labels"])
            if want is None or not eager:
                assert not got
            else:
                assert len(got) >= 2 and all(d[2] == min_scores and d[5] == want[0] for d in got), got
            n += len(got)
    assert (n == 0) == (want is None)


@pytest.fixture(scope="module")
def moving():
    """per stream of the moving set: (model, pcm, the oracle's logits)"""
    models, pcm = R.moving_models(), R.moving_pcm()
    assert pcm.shape == (R.MOVING_STREAMS, R.MOVING_CHUNKS * 480) and R.MOVING_STREAMS <= 6 and R.MOVING_CHUNKS <= 100
    return [(models[mi], pcm[s], oracle_logits(models[mi], pcm[s])) for s, mi in enumerate(R.MOVING_STREAM_MODEL)]


@pytest.mark.parametrize("two_layers", [False, True])
@pytest.mark.parametrize("eager,min_scores", [(False, 1), (False, 3), (True, 3)])
@pytest.mark.parametrize("avg_threshold", [0.0, R.MOVING_AVG_THRESHOLD])
def test_moving_models_against_the_oracle(moving, avg_threshold, eager, min_scores, two_layers):
    cfg = R.Cfg(R.MOVING_THRESHOLD, avg_threshold, min_scores, eager)
    n = 0
    for s, (model, pcm, lg) in enumerate(moving):
        if two_layers:   # the form a .rpw file can hold (the single-stream detector's tests)
            model = R.moving_models(True)[R.MOVING_STREAM_MODEL[s]]
            lg = oracle_logits(model, pcm)
        got = R.detect_model_ref(lg, model["train_size"], 0, cfg)
        same_as_oracle(got, oracle_run(model, pcm, cfg), model["labels"])
        n += len(got)
    assert n >= 3 * R.MOVING_STREAMS


@pytest.mark.parametrize("two_layers", [False, True])
@pytest.mark.parametrize("avg_threshold", [0.0, R.MOVING_AVG_THRESHOLD])
def test_moving_set_conditions(moving, avg_threshold, two_layers):
    """what tests/test_gpu_nn_decide.py relies on (not eager, min_scores 1): every stream has 3 detections or more; 2 or more have a
    counter of 2 or more; 2 or more have a best window whose label is not that of their first or of their last passing window; no window's
    f64 score or avg score lies within 1e-4 of its threshold -- 100 times the 1e-6 tests/test_gpu_model_pin.py allows this formula on the
    device, so the device's logits (its forward is within that bar of the oracle's) decide every window the same way"""
    cfg = R.Cfg(R.MOVING_THRESHOLD, avg_threshold, 1, False)
    counters, other_label, labels, nearest = 0, 0, set(), np.inf
    for s, (model, pcm, lg) in enumerate(moving):
        if two_layers:
            model = R.moving_models(True)[R.MOVING_STREAM_MODEL[s]]
            lg = oracle_logits(model, pcm)
        L = model["train_size"]
        assert np.abs(lg).max() < 10
        det = R.detect_model_ref(lg, L, 0, cfg)
        assert len(det) >= 3, (s, det)
        agg, avg, lab = R.window_rows(lg, 0, cfg)
        for d, wins in zip(det, R.detection_windows(det, agg, L)):
            assert len(wins) == d[2] and d[1] in wins and lab[d[1]] == d[5], (s, d, wins)
            assert agg[d[1]] == max(agg[w] for w in wins)
            counters += d[2] >= 2
            other_label += lab[wins[0]] != d[5] or lab[wins[-1]] != d[5]
            labels.add(int(d[5]))
        for w in range(len(lg)):
            f64 = R.decide_f64(lg[w], 0, cfg.score_ref, avg_threshold)
            if f64 is not None:
                nearest = min(nearest, abs(f64[1] - R.MOVING_THRESHOLD))
                if avg_threshold != 0.0:
                    nearest = min(nearest, abs(f64[2] - avg_threshold))
    print("avg_threshold %g: %d detections with a counter of 2 or more, %d whose first or last window has another label, labels %s, "
          "nearest score to a gate %.3g" % (avg_threshold, counters, other_label, sorted(labels), nearest))
    assert counters >= 2 and other_label >= 2 and labels == {1, 2}
    assert nearest > 1e-4


def test_minus_zero_cannot_leave_the_forward():
    """total_cmp puts -0 below +0, the only place where it and `<` disagree on finite values.  The forward cannot produce a -0 logit from
    the biases used here: every kernel's accumulator starts at +0 (mlp_tail_layers: s0 = s1 = 0.f, then (s0 + s1) + bias), +0 + x is +0
    for x = -0 and x otherwise, so a logit is -0 only if the bias is -0 -- and none is.  The +-0 ordering of total_cmp is therefore NOT
    driven on the device; the reference and test_total_cmp_key_orders_like_f32_total_cmp hold it."""
    biases = [v[0] for v in R.CONSTANT.values()] + [R.NAN_VECTOR[0]] + [np.array(m[4], F32) for m in R.MOVING]
    for b in biases:
        for acc in (F32(0.0), F32(0.0) + F32(-0.0), F32(0.0) * F32(-3.0) + F32(0.0)):
            out = (np.full(len(b), acc, F32) + b).astype(F32)
            assert not np.any(np.signbit(out) & (out == 0)), b
            keep = ~np.isnan(b)
            assert np.array_equal(out[keep].view(np.uint32), b[keep].view(np.uint32))
    assert np.signbit(F32(-0.0) + F32(-0.0)) and not np.signbit(F32(0.0) + F32(-0.0))


def test_nan_logit():
    """[c, NaN, a] with none 0: under total_cmp the positive NaN is the maximum, so the label is 1, both scores are NaN, >= fails and nothing
    is reported -- not label 2, which `<` on floats would move on to.  The oracle's loop follows the same rule."""
    bias, none_index = R.NAN_VECTOR
    assert R.get_label(bias) == 1
    for avg_threshold in (0.0, 0.2):
        assert R.decide(bias, none_index, 0.22, -1.0, avg_threshold) is None
        f64 = R.decide_f64(bias, none_index, 0.22, avg_threshold)
        assert f64[0] == 1 and np.isnan(f64[1])
    # second_prob with a NaN label: == filters nothing, the minimum under total_cmp is c
    assert R._probs(bias, none_index, 0.2)[3] == R.C
    # a NaN that is not the label: [NaN, a, b] with none 0 -> the NaN is the maximum and the none label: no detection
    assert R.decide(np.array([np.nan, R.A, R.B], F32), 0, 0.22, -1.0, 0.2) is None
    # a negative NaN is the smallest value: label 2, second is the NaN, avg NaN -> nothing with an avg gate, a detection without
    neg = np.array([R.C, -np.nan, R.A], F32)
    neg[1] = np.array([0xFFC00000], np.uint32).view(F32)[0]
    assert R.get_label(neg) == 2 and R.decide(neg, 0, 0.22, 0.2, 0.2) is None and R.decide(neg, 0, 0.22, 0.2, 0.0)[0] == 2
    pcm = R.noise_pcm(1, CONST_CHUNKS)[0]
    for vec in (bias, neg):
        for hidden in ((), (3,)):
            model = R.constant_model(vec, none_index, 20, hidden)
            for avg_threshold in (0.0, 0.2):
                cfg = R.Cfg(CONST_THRESHOLD, avg_threshold, 1, True)
                lg = np.tile(vec, (3 * CONST_CHUNKS - 3 - 20 + 1, 1))
                got = R.detect_model_ref(lg, 20, none_index, cfg)
                same_as_oracle(got, oracle_run(model, pcm, cfg), model["labels"])
                assert bool(got) == (vec is neg and avg_threshold == 0.0)
