"""What the mixed-set tests share (tests/test_gpu_mixed_sets.py, tests/test_mixed_set_cases.py): streams that hold wakeword references of a
wakeword bank AND models of a model bank on one detector.

The models, their thresholds and the bursts are tests/model_set_cases.py's: windows of 30 / 47 / 96 / 195 frames.  The wakeword bank is at
mfcc_size 16 and holds three references enrolled from one utterance U, a stretch of nn_decide_ref.moving_audio with four bursts: its first 42
frames (shorter than every model but the 30-frame one), its first 120 (between 96 and 195; two templates and their average, so the
averaged-template test runs) and all 207 (longer than every model).  Every stream is its own moving_audio with U written over it at its own
chunk, so the references fire where U ends inside the stream's window and the models fire on the bursts around it.  The references carry
thresholds of their own (REF_THRESHOLD), which keeps them to U and lets both kinds win.

ROWS (ref_set_size 2, model_set_size 2) are the issue's: reference only, model only, short reference + long model, long reference + short
model, the reference longer than every model + a model, two + two, all -1, duplicates, a hole in front of a live slot on each side.  Audio,
offsets and thresholds were chosen on the CPU with oracle.rp_oracle.Detector (add_ref ... then add_model ...); check_inputs() asserts on the
ORACLE's output that they show the feature."""
import ctypes as C
from collections import OrderedDict

import numpy as np

import model_set_cases as M
import nn_decide_ref as R
from oracle import rp_oracle as orc

F32 = np.float32
K = 16
CHUNKS = M.CHUNKS            # 4 s
REF_CHUNKS = (15, 41, 70)    # -> 42, 120 and 207 frames
REF_LENS = tuple(3 * c - 3 for c in REF_CHUNKS)
REF_THRESHOLD = (0.6, 0.6, 0.6)
REF_AVG_THRESHOLD = (None, 0.3, None)
# rows: (reference slots, model slots, the chunk U starts at, the L of the stream's moving_audio)
ROWS = [
    ((0, 1), (-1, -1), 20, 40),      # reference only
    ((-1, -1), (0, 3), 30, 50),      # model only
    ((0, -1), (3, -1), 4, 60),       # short reference + long model
    ((1, -1), (0, -1), 52, 70),      # long reference + short model
    ((2, -1), (1, -1), 0, 80),       # the reference longer than every model + a model
    ((0, 1), (1, 2), 28, 90),        # two + two
    ((-1, -1), (-1, -1), 22, 100),   # all -1
    ((0, 0), (1, 1), 4, 110),        # duplicates
    ((-1, 1), (-1, 2), 12, 120),     # a hole in front of a live slot on each side
    ((1, 0), (3, 0), 40, 45),        # two + two, the longest last on the reference side and first on the model side
]
S = len(ROWS)
REF_ROWS = np.array([r[0] for r in ROWS], np.int32)
MODEL_ROWS = np.array([r[1] for r in ROWS], np.int32)


def utterance():
    """U: 70 chunks of moving_audio with bursts at frames 7, 57, 107 and 157"""
    return R.moving_audio(20, 0, 19 + REF_CHUNKS[2])[19 * 480:]


def pcm(n_chunks=CHUNKS):
    """[S][n_chunks * 480]: every stream its own bursts, U written over them from its own chunk on"""
    u = utterance()
    out = []
    for s, (_, _, at, L) in enumerate(ROWS):
        x = R.moving_audio(30 + s, L, n_chunks).copy()
        n = min(len(u), len(x) - at * 480)
        x[at * 480:at * 480 + n] = u[:n]
        out.append(x)
    return np.stack(out)


_REFS = []


def refs():
    """the three references as oracle.rp_oracle.Detector.add_ref takes them"""
    if not _REFS:
        u = utterance()
        rng = np.random.default_rng(7)
        for i, nch in enumerate(REF_CHUNKS):
            sf = OrderedDict([("t0", orc.wav_features(u[:nch * 480], 16000, K))])
            avg = None
            if REF_AVG_THRESHOLD[i] is not None:   # a second recording of the same stretch: a little noise on top
                noisy = (u[:nch * 480] + rng.standard_normal(nch * 480) * 2e-4).astype(F32)
                sf["t1"] = orc.wav_features(noisy, 16000, K)
                avg = orc.average_templates(sf)
            assert sf["t0"].shape == (REF_LENS[i], K)
            _REFS.append({"name": "ref%d" % i, "samples_features": sf, "avg_features": avg, "threshold": REF_THRESHOLD[i],
                          "avg_threshold": REF_AVG_THRESHOLD[i], "rms_level": float("nan")})
    return _REFS


def bank_wakewords():
    """the references as rustpotter_amd.WakewordBank(wakewords=...) takes them"""
    return [(list(r["samples_features"].values()), r["avg_features"], r["threshold"], r["avg_threshold"]) for r in refs()]


_MODELS = []


def model_dicts():
    if not _MODELS:
        _MODELS.extend(M.model_dict(i, ws, bs) for i, (ws, bs) in enumerate(M.bank_weights()))
    return _MODELS


def lmax_of(ref_row, model_row):
    return max([0] + [REF_LENS[w] for w in ref_row if w >= 0] + [M.MODELS[m][0] for m in model_row if m >= 0])


def oracle_kwargs(cfg):
    """a rustpotter_amd.DetectorConfig (or anything with its fields) as oracle.rp_oracle.Detector's arguments"""
    vad = getattr(cfg, "vad_mode", None)
    vad = {0: None, 1: "easy", 2: "medium", 3: "hard"}[int(vad)] if vad is not None and not isinstance(vad, str) else vad
    mode = getattr(cfg, "score_mode", "max")
    mode = mode if isinstance(mode, str) else {0: "average", 1: "max", 2: "median", 3: "p25", 4: "p50", 5: "p75", 6: "p80", 7: "p90", 8: "p95"}[int(mode)]
    return dict(avg_threshold=cfg.avg_threshold, threshold=cfg.threshold, min_scores=cfg.min_scores, eager=bool(cfg.eager),
                score_ref=getattr(cfg, "score_ref", 0.22), band_size=getattr(cfg, "band_size", 5), score_mode=mode, vad_mode=vad)


def oracle_detect(ref_row, model_row, x, cfg, ref_levels=None, model_levels=None, **filters):
    """Rustpotter::new(config), add_wakeword per live reference slot in slot order, then per live model slot in slot order, then
    process_samples per 30 ms chunk -> [(chunk, kind "ref" / "model", bank index, label or -1, score, avg_score, counter)]"""
    kw = oracle_kwargs(cfg)
    kw.update(filters)
    d = orc.Detector(**kw)
    who = []
    for w in ref_row:
        if w >= 0:
            r = dict(refs()[w])
            if ref_levels is not None:
                r["rms_level"] = float(ref_levels[w])
            d.add_ref(r)
            who.append(("ref", int(w)))
    for m in model_row:
        if m >= 0:
            md = dict(model_dicts()[m])
            if model_levels is not None:
                md["rms_level"] = float(model_levels[m])
            d.add_model(md)
            who.append(("model", int(m)))
    out = []
    x = np.ascontiguousarray(x, F32)
    for i in range(0, len(x) - 479, 480):
        det = orc.Detection()
        if orc.lib().orc_detector_process(d._h, x[i:i + 480].ctypes.data_as(C.POINTER(C.c_float)), C.byref(det)):
            kind, idx = who[det.wakeword]
            out.append((i // 480, kind, idx, int(det.name) if kind == "model" else -1, F32(det.score), F32(det.avg_score), int(det.counter)))
    return out


class Cfg:
    """the fields of a DetectorConfig the oracle reads"""

    def __init__(self, threshold=M.THRESHOLD, avg_threshold=M.AVG_THRESHOLD, min_scores=2, eager=True, score_ref=0.22, band_size=5,
                 score_mode="max", vad_mode=None):
        self.threshold, self.avg_threshold, self.min_scores, self.eager = threshold, avg_threshold, min_scores, eager
        self.score_ref, self.band_size, self.score_mode, self.vad_mode = score_ref, band_size, score_mode, vad_mode


def check_inputs(want, alone):
    """want[s]: the oracle's detections of row s; alone[s]: (those of its reference slots alone, those of its model slots alone).  The inputs
    show the feature: references win beside live models, models beside live references, both in one stream, and one detector differs from
    the union of two."""
    key = lambda d: (d[0], d[1], d[2], d[3], d[6])
    both = [s for s, (rr, mr, _, _) in enumerate(ROWS) if max(rr) >= 0 and max(mr) >= 0]
    ref_wins = sum(1 for s in both for d in want[s] if d[1] == "ref")
    model_wins = sum(1 for s in both for d in want[s] if d[1] == "model")
    both_kinds = [s for s in both if {d[1] for d in want[s]} == {"ref", "model"}]
    differ = [s for s in both if sorted(map(key, want[s])) != sorted(map(key, alone[s][0] + alone[s][1]))]
    assert ref_wins >= 2, ref_wins
    assert model_wins >= 2, model_wins
    assert both_kinds, "no stream in which both kinds win a detection"
    assert differ, "no stream whose detections differ from the union of a reference-only and a model-only detector"
    return ref_wins, model_wins, both_kinds, differ
