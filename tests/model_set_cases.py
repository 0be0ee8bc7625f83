"""What the model-set tests share (tests/test_gpu_model_bank_sets.py, tests/test_gpu_stream_model_bank_sets.py): the bank, the rows of sets,
the audio and the host fold a detection is held against.

The bank: six models at mfcc_size 16 -- windows of 30, 47 (odd: half a k-block of zeros), 96 and 195 frames; layer 1 of 8 / 3 / 13 (one
16-output tile) and 20 / 32 (two); one, two and three layers; two and three labels; none_index 0, last and -1; model 5 holds the parameters
of model 0 (the twin pair).  The last layer is scaled by GAIN and the bias of "none" is set per model (NONE_BIAS), so that on the bursts of
nn_decide_ref.moving_audio the scores move through the threshold: chosen on the CPU with the oracle's forward (tools: this module's
fold_ref over oracle.rp_oracle.mlp_forward of oracle.rp_oracle.mfcc_stream's frames).

The rows (S = 9, set_size 3): [a,-1,-1], [a,b,-1] with L_a != L_b, [b,a,-1], [-1,a,-1], all -1, [a,a,b], the twins in both orders, and a
row of three different windows led by the model without a "none" label."""
import numpy as np

import nn_decide_ref as R
from scan_ref import scan_ref, vad_values_ref

F32 = np.float32
K = 16
# (train_size L, hidden widths, labels, none_index)
MODELS = [(30, (8,), 2, 0), (47, (20, 12), 3, 0), (96, (), 3, 2), (195, (32, 16), 2, 0), (195, (13,), 2, -1), (30, (8,), 2, 0)]
NONE_INDEX = [m[3] for m in MODELS]
TWINS = (0, 5)
SETS = np.array([[0, -1, -1], [0, 3, -1], [3, 0, -1], [-1, 1, -1], [-1, -1, -1], [1, 1, 2], [0, 5, -1], [5, 0, -1], [4, 2, 1]], np.int32)
S, SET_SIZE = SETS.shape
LABEL_PITCH = 3
SEED, GAIN = 11, 3.0
# the last layer's bias of the "none" label (model 4 has none: the bias of its label 0, which the scores of label 1 are taken against 0 of)
NONE_BIAS = [0.3, 0.6, 0.3, 0.2, -0.4, 0.3]
THRESHOLD, AVG_THRESHOLD = 0.5, 0.3
CHUNKS = 133    # 4 s


def bank_weights():
    """[(ws, bs)] of the six models: W_l [out][in] scaled by 1 / sqrt(in), biases 0.1 N(0, 1), the last layer times GAIN"""
    rng = np.random.default_rng(SEED)
    out = []
    for i, (L, hidden, nl, none) in enumerate(MODELS):
        dims = [L * K] + list(hidden) + [nl]
        ws = [(rng.standard_normal((dims[j + 1], dims[j])) / np.sqrt(dims[j])).astype(F32) for j in range(len(dims) - 1)]
        bs = [(rng.standard_normal(dims[j + 1]) * 0.1).astype(F32) for j in range(len(dims) - 1)]
        ws[-1] = (ws[-1] * F32(GAIN)).astype(F32)
        bs[-1][none if none >= 0 else 0] = F32(NONE_BIAS[i])
        out.append((ws, bs))
    out[TWINS[1]] = ([w.copy() for w in out[TWINS[0]][0]], [b.copy() for b in out[TWINS[0]][1]])
    return out


def model_dict(i, ws, bs):
    """model i as oracle.rp_oracle.Detector.add_model takes it"""
    weights = {}
    for l, (w, b) in enumerate(zip(ws, bs)):
        weights["ln%d.weight" % (l + 1)] = w
        weights["ln%d.bias" % (l + 1)] = b
    return {"labels": R.labels_for(MODELS[i][2], MODELS[i][3]), "train_size": MODELS[i][0], "mfcc_size": K,
            "m_type": {2: "tiny", 3: "small"}.get(len(ws)), "weights": weights, "rms_level": float("nan")}


def pcm(n_chunks=CHUNKS):
    """[S][n_chunks * 480]: bursts of coloured noise over faint white noise, every stream its own"""
    return np.stack([R.moving_audio(s, 40 + 10 * s, n_chunks) for s in range(S)])


def lmax_of(row):
    return max([0] + [MODELS[mi][0] for mi in row if mi >= 0])


def n_win_of(nf, row):
    lm = lmax_of(row)
    return max(nf - lm + 1, 0) if lm else 0


def synth_mfcc(rng, n_streams, nf):
    """rows with coefficient-dependent offsets about ten times their spread and a slow drift"""
    off = rng.uniform(-30.0, 30.0, K).astype(F32)
    drift = np.linspace(0.0, 1.0, nf)[None, :, None] * rng.uniform(-6.0, 6.0, (n_streams, 1, K))
    return (rng.standard_normal((n_streams, nf, K)) * rng.uniform(0.5, 2.0, (n_streams, 1, 1)) + off + drift).astype(F32)


def fold_ref(logits, row, nf, cfg, mfcc=None, fpf=3):
    """The detections of ONE stream that holds the set `row`, from its logits [set_size][>= n_win_s][label pitch] (row (j, w): slot j on the
    window that starts at frame w): per window every live slot decides as WakewordNN::run_detection does (nn_decide_ref.window_rows), the
    best passing score wins, the first slot of equals (run_wakeword_detectors); then the state machine (scan_ref) with the window Lmax and
    the countdown Lmax / 2.  mfcc: the stream's frames when cfg.vad_mode is set.
    -> [(frame, window, counter, avg_score, score, (bank index, label))]"""
    lm = lmax_of(row)
    n_win = n_win_of(nf, row)
    if n_win == 0:
        return []
    best, bavg, who = np.full(n_win, -2.0, F32), np.zeros(n_win, F32), [None] * n_win
    for j, mi in enumerate(row):
        if mi < 0:
            continue
        agg, avg, lab = R.window_rows(logits[j, :n_win, :MODELS[mi][2]], NONE_INDEX[mi], cfg)
        for w in range(n_win):
            if agg[w] != F32(-2.0) and (who[w] is None or agg[w] > best[w]):
                best[w], bavg[w], who[w] = agg[w], avg[w], (int(mi), int(lab[w]))
    vad = getattr(cfg, "vad_mode", None)
    vv, mode_value = None, 0.0
    if vad:
        vv, mode_value = vad_values_ref(mfcc[:nf]), R.VAD_MODE_VALUE[vad]
    return scan_ref(best, bavg, nf, lm, -1.0, -1.0, cfg.min_scores, cfg.eager, vv, mode_value, fpf=fpf, label=who)


def bits(x):
    return int(F32(x).view(np.uint32))
