"""What a wakeword model's detector does AFTER the logits, in plain Python, and models that steer chosen logits into it.

The decision stage -- the label rule, the two scores, the two gates, the label that travels with a partial detection -- is restated here
from the Rust source alone: WakewordNN::get_label / run_detection_by_label / validate_scores / calc_inverse_similarity
(src/wakewords/nn/wakeword_nn.rs:47-163) and the partial-detection update of Rustpotter::run_detection (src/detector.rs:398-432, which
tests/scan_ref.py walks).  It is NOT restated from oracle/rp_oracle.c or from the kernels, whose loops are copies of each other:
nn_score_kernel, nn_score_bank_kernel, nn_score_bank_stream_kernel (rp_mlp.hip), the host loop of rp_detector.cpp and the oracle's
nn_run_detection are all judged by it (tests/test_nn_decide_ref.py on the CPU, tests/test_gpu_nn_decide.py on the device).

Every value is np.float32; comparisons are f32 comparisons, orderings go through the integer key of f32::total_cmp.

Steered models.  A model whose LAST layer has all-zero weights answers that layer's bias, bit for bit, for every window of any audio
(an accumulator that starts at +0 gains only +-0 products, and +0 + b == b): constant_model().  moving_model() has one layer of three
labels, "none" first: label 1 weighs coefficient 0 of the window's last frame, label 2 coefficient 0 of an earlier frame, so a burst of
low-passed noise on faint white noise (moving_audio) lifts label 1 when it enters the window and label 2 when it reaches that earlier
frame -- the window is mean-normalised -- and one detection gathers windows of both labels.
"""
import numpy as np

from scan_ref import scan_ref

F32 = np.float32
K = 16
VAD_MODE_VALUE = {"easy": 2.0, "medium": 2.5, "hard": 3.0}   # VADMode::get_value, src/config.rs:140-146


# ------------------------------------------------------------------ the decision of one window
def total_cmp_key(x):
    """the integer f32::total_cmp compares: the bits as i32, the low 31 flipped when the sign is set.  -NaN < -inf < ... < -0 < +0 < ...
    < +inf < +NaN"""
    b = int(np.array(x, F32).view(np.int32))
    return b ^ 0x7FFFFFFF if b < 0 else b


def get_label(logits):
    """iter().enumerate().max_by(total_cmp): Iterator::max_by returns the LAST of several equal maxima"""
    best = 0
    for i in range(1, len(logits)):
        if total_cmp_key(logits[i]) >= total_cmp_key(logits[best]):
            best = i
    return best


def inverse_similarity(n1, n2, reference):
    """calc_inverse_similarity, every operation in f32"""
    n1, n2, reference = F32(n1), F32(n2), F32(reference)
    with np.errstate(over="ignore", invalid="ignore"):
        return F32(1) - (F32(1) / (F32(1) + np.exp(F32(F32(F32(n1 - n2) - reference) / reference), dtype=F32)))


def inverse_similarity_f64(n1, n2, reference):
    """the same formula in f64 on the f32 inputs: what a score is held against, and what says how far a window is from a gate"""
    n1, n2, reference = float(F32(n1)), float(F32(n2)), float(F32(reference))
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 - 1.0 / (1.0 + np.exp(((n1 - n2) - reference) / reference))


def score_reference(score_ref):
    """WakewordNN::new: score_ref * 10., an f32 product"""
    return F32(F32(score_ref) * F32(10))


def _probs(logits, none_index, avg_threshold):
    """-> (label, label_prob, none_prob, second_prob or None when the avg score is not computed)"""
    logits = [F32(v) for v in logits]
    label = get_label(logits)
    label_prob = logits[label]
    none_prob = logits[none_index] if none_index >= 0 else F32(0)       # scores.get(NN_NONE_LABEL).unwrap_or(&0.)
    second = None
    if F32(avg_threshold) != F32(0):                                    # run_detection: calc_avg_score = avg_threshold != 0.
        rest = [p for p in logits if not (label_prob == p)]             # .filter(|p| !label_prob.eq(*p)): f32 ==, so a NaN stays in
        second = F32(0)                                                 # .unwrap_or(&0.)
        if rest:
            second = rest[0]
            for p in rest[1:]:                                          # .max_by(|a, b| b.total_cmp(a)): the smallest, the last of equals
                if total_cmp_key(p) <= total_cmp_key(second):
                    second = p
    return label, label_prob, none_prob, second


def decide(logits, none_index, score_ref, threshold, avg_threshold):
    """one window: None, or (label, score, avg_score) of the detection WakewordNN::run_detection returns"""
    label, label_prob, none_prob, second = _probs(logits, none_index, avg_threshold)
    if label == none_index:
        return None
    ref = score_reference(score_ref)
    avg_score = F32(0) if second is None else inverse_similarity(label_prob, second, ref)
    score = inverse_similarity(label_prob, none_prob, ref)
    if score >= F32(threshold) and avg_score >= F32(avg_threshold):    # validate_scores: >= twice; false for a NaN
        return label, score, avg_score
    return None


def decide_f64(logits, none_index, score_ref, avg_threshold):
    """-> None for the none label, else (label, score, avg_score) with the scores evaluated in f64 and NO gate applied"""
    label, label_prob, none_prob, second = _probs(logits, none_index, avg_threshold)
    if label == none_index:
        return None
    ref = score_reference(score_ref)
    return label, inverse_similarity_f64(label_prob, none_prob, ref), (0.0 if second is None else inverse_similarity_f64(label_prob, second, ref))


class Cfg:
    """the fields of a DetectorConfig the decision reads (rustpotter_amd.DetectorConfig has the same names)"""

    def __init__(self, threshold=0.5, avg_threshold=0.0, min_scores=1, eager=False, score_ref=0.22, vad_mode=None):
        self.threshold, self.avg_threshold, self.min_scores, self.eager = threshold, avg_threshold, min_scores, eager
        self.score_ref, self.vad_mode = score_ref, vad_mode


def window_rows(logits, none_index, cfg):
    """-> (agg, avg, label) rows: decide() per window, agg -2 where it answers None (no score is negative, the scan asks for > -1)"""
    n = len(logits)
    agg, avg, lab = np.full(n, -2.0, F32), np.zeros(n, F32), np.full(n, -1, np.int64)
    for w in range(n):
        d = decide(logits[w], none_index, cfg.score_ref, cfg.threshold, cfg.avg_threshold)
        if d is not None:
            lab[w], agg[w], avg[w] = d
    return agg, avg, lab


def detect_model_ref(logits, L, none_index, cfg, vad_values=None, fpf=3):
    """logits [n_win][n_labels] of ONE stream, row w the window of L frames that starts at frame w -> the stream's detections
    [(frame, window, counter, avg_score, score, label)].  The gates are decide()'s; the state machine is scan_ref's, which only has to see
    which windows passed (thresholds -1), with the wakeword's window length and Rustpotter's countdown of L / 2 frames."""
    agg, avg, lab = window_rows(logits, none_index, cfg)
    vad_mode = getattr(cfg, "vad_mode", None)
    mode_value = 0.0
    if vad_values is not None:
        mode_value = VAD_MODE_VALUE[vad_mode if isinstance(vad_mode, str) else {1: "easy", 2: "medium", 3: "hard"}[int(vad_mode)]]
    return scan_ref(agg, avg, len(logits) + L - 1, L, -1.0, -1.0, cfg.min_scores, cfg.eager, vad_values, mode_value, fpf=fpf, label=lab)


# ------------------------------------------------------------------ steered models
A, B, C = F32(2.5), F32(0.75), F32(-1.25)    # a > b > c, |x| < 4, exact in f32


def _wide():
    """32 labels, the model bank's widest label row: the maximum at 7 and again at 31, the rest below b"""
    v = np.random.default_rng(32).uniform(-3.0, 0.5, 32).astype(F32)
    v[7] = v[31] = A
    return v


def _f(d):
    """the score of a logit difference d (f64) at the default score_ref"""
    ref = float(score_reference(0.22))
    return 1.0 - 1.0 / (1.0 + np.exp((d - ref) / ref))


# name -> (bias vector, none_index, expected (label, second or None: "nothing left") or None: never a detection)
CONSTANT = {
    "aa_none0": (np.array([A, A], F32), 0, (1, None)),
    "aa_none1": (np.array([A, A], F32), 1, None),
    "aa_nonone": (np.array([A, A], F32), -1, (1, None)),
    "baa_none0": (np.array([B, A, A], F32), 0, (2, B)),
    "abc_none2": (np.array([A, B, C], F32), 2, (0, C)),
    "cab_none0": (np.array([C, A, B], F32), 0, (1, C)),
    "a_nonone": (np.array([A], F32), -1, (0, None)),
    "a_none0": (np.array([A], F32), 0, None),
    "wide32_none0": (_wide(), 0, (31, F32(_wide().min()))),
}
NAN_VECTOR = (np.array([C, np.nan, A], F32), 0)     # np.nan: a positive quiet NaN, the largest value under total_cmp
# not in the table: its own windows are the none label; a row of ZERO logits (what lies behind a short stream's windows in a bank call)
# would be label 1 with the score of equal logits, 0.2689
QUIET_VECTOR = (np.array([A, C], F32), 0)
# name -> (window length, hidden widths) of the model that answers the vector on the device: L 20 and 40, one layer and two
CONSTANT_SHAPES = {
    "aa_none0": (20, ()), "aa_none1": (40, ()), "aa_nonone": (20, (3,)), "baa_none0": (40, (3,)), "abc_none2": (20, ()),
    "cab_none0": (40, (5,)), "a_nonone": (20, (3,)), "a_none0": (20, ()), "wide32_none0": (40, ()), "nan": (40, ()), "quiet": (40, (3,)),
}


def constant_vector(name):
    """-> (bias, none_index) of a table entry, of the NaN vector ("nan") or of the quiet one ("quiet")"""
    return NAN_VECTOR if name == "nan" else QUIET_VECTOR if name == "quiet" else CONSTANT[name][:2]


def expected_constant(name, avg_threshold):
    """the table's decision in numbers: None, or (label, f64 score, f64 avg score)"""
    bias, none_index, want = CONSTANT[name]
    if want is None:
        return None
    label, second = want
    none_prob = float(bias[none_index]) if none_index >= 0 else 0.0
    a = float(bias[label])
    return label, _f(a - none_prob), (0.0 if F32(avg_threshold) == 0 else _f(a - (0.0 if second is None else float(second))))


def labels_for(n_labels, none_index):
    return ["none" if i == none_index else "l%d" % i for i in range(n_labels)]


def _model(L, ws, bs, none_index):
    weights = {}
    for l, (w, b) in enumerate(zip(ws, bs)):
        weights["ln%d.weight" % (l + 1)] = np.ascontiguousarray(w, F32)
        weights["ln%d.bias" % (l + 1)] = np.ascontiguousarray(b, F32)
    # m_type: what a .rpw file of it says (Tiny: two layers, the others three); a one-layer model has no file form
    return {"labels": labels_for(len(bs[-1]), none_index), "train_size": L, "mfcc_size": K, "m_type": {2: "tiny", 3: "small"}.get(len(ws)),
            "weights": weights, "rms_level": float("nan"), "none_index": none_index, "ws": [weights["ln%d.weight" % (l + 1)] for l in range(len(ws))],
            "bs": [weights["ln%d.bias" % (l + 1)] for l in range(len(ws))]}


def constant_model(bias, none_index, L, hidden=(), seed=0):
    """layers L * 16 -> hidden... -> len(bias); the hidden layers random, the last layer zero weights and `bias`"""
    rng = np.random.default_rng(seed)
    dims = [L * K] + list(hidden) + [len(bias)]
    ws = [(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(F32) for i in range(len(dims) - 1)]
    bs = [(rng.standard_normal(dims[i + 1]) * 0.1).astype(F32) for i in range(len(dims) - 1)]
    ws[-1] = np.zeros_like(ws[-1])
    bs[-1] = np.array(bias, F32)
    return _model(L, ws, bs, none_index)


def moving_model(L, early, g1, g2, bias, two_layers=False):
    """three labels, none = 0: logit 1 = g1 x[L - 1][0] + bias[1], logit 2 = g2 x[early][0] + bias[2], logit 0 = bias[0], x the
    mean-normalised window.  two_layers: the same through a hidden layer of four, relu(x) - relu(-x) (a .rpw file holds two layers or three)"""
    sel = np.zeros((2, L * K), F32)
    sel[0, (L - 1) * K] = 1
    sel[1, early * K] = 1
    if not two_layers:
        w = np.zeros((3, L * K), F32)
        w[1], w[2] = F32(g1) * sel[0], F32(g2) * sel[1]
        return _model(L, [w], [np.array(bias, F32)], 0)
    w1 = np.stack([sel[0], -sel[0], sel[1], -sel[1]]).astype(F32)
    w2 = np.zeros((3, 4), F32)
    w2[1, :2] = (g1, -g1)
    w2[2, 2:] = (g2, -g2)
    return _model(L, [w1, w2], [np.zeros(4, F32), np.array(bias, F32)], 0)


# The moving set, fixed on the CPU by tests/test_nn_decide_ref.py: (L, early frame, g1, g2, bias)
MOVING = [
    (20, 6, 0.10, 0.22, (0.0, -1.0, -1.0)),
    (40, 24, 0.12, 0.10, (0.0, -1.0, -1.0)),
]
MOVING_THRESHOLD, MOVING_AVG_THRESHOLD = 0.42, 0.345
MOVING_CHUNKS = 100           # 3 s
MOVING_STREAMS = 6


def moving_audio(stream, L, n_chunks=MOVING_CHUNKS):
    """[n_chunks * 480] f32: faint white noise with bursts of low-passed noise (a moving average over `taps` samples), each burst with its
    own level, colour, length and distance to the next.  The MFCC front end follows the colour of a frame, not its level: coefficient 0
    sits near -60 in the white noise and between -35 and -15 in a burst"""
    rng = np.random.default_rng(1000 + stream)
    n = n_chunks * 480
    x = rng.standard_normal(n) * 1e-4
    burst, gap = 10 * 160, (40 + L) * 160
    at = (L + 4 + 3 * stream) * 160
    while at + 2 * burst < n:
        length = int(burst * rng.uniform(0.8, 1.2))
        taps = int(rng.integers(3, 17))
        noise = np.convolve(rng.standard_normal(length + taps - 1), np.ones(taps) / np.sqrt(taps), "valid")
        x[at:at + length] += noise * rng.uniform(0.05, 0.3)
        at += length + int(gap * rng.uniform(1.0, 1.05))
    return x.astype(F32)


MOVING_STREAM_MODEL = [0, 1, 0, 1, 0, 1]     # stream s of the moving set runs MOVING[MOVING_STREAM_MODEL[s]]


def moving_models(two_layers=False):
    return [moving_model(*m, two_layers=two_layers) for m in MOVING]


def moving_pcm():
    """[MOVING_STREAMS][MOVING_CHUNKS * 480]: stream s hears bursts spaced for the window length of its model"""
    return np.stack([moving_audio(s, MOVING[MOVING_STREAM_MODEL[s]][0]) for s in range(MOVING_STREAMS)])


def noise_pcm(n_streams, n_chunks, seed=7):
    """what the constant models hear (they answer their bias whatever it is): white noise, each stream at its own level"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_streams, n_chunks * 480)) * rng.uniform(0.01, 0.2, (n_streams, 1))).astype(F32)


def detection_windows(det, agg, L, fpf=3):
    """per detection of detect_model_ref the passing windows it counted: those between the previous detection's reset (the extractor
    starts again with the next chunk) and the frame that returned it"""
    out, start = [], 0
    for d in det:
        out.append([w for w in range(start, d[0] - L + 1) if agg[w] > -1])
        start = fpf * ((d[0] + 3) // fpf + 1)
    return out
