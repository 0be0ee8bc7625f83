"""Pins tests/scan_ref.py -- the plain-Python state machine the GPU scan is compared with (tests/test_gpu_scan_edges.py) -- to the
oracle's chunk-by-chunk detector on the reference's simulation stream: same chunks, counters and, bit for bit, scores."""
import json
import os

import numpy as np
import pytest

import rpw_py
import simstream
from oracle import rp_oracle as orc
from scan_ref import scan_ref, vad_values_ref

G = simstream.GOLDEN
EXP = json.load(open(os.path.join(G, "expectations.json")))
VAD_MODE_VALUE = {"easy": 2.0, "medium": 2.5, "hard": 3.0}   # VADMode::get_value, src/config.rs:140-146


@pytest.fixture(scope="module")
def sim():
    s = simstream.simulation_stream_i16()
    return s, orc.mfcc_stream(simstream.i16_to_f32(s), 5)


@pytest.mark.parametrize("case", ["max", "median", "ignore_alexa", "vad_easy"])
def test_scan_ref_equals_the_chunked_detector(sim, case):
    s, mf = sim
    e = EXP["simulation"][case]
    w = rpw_py.load_rpw(os.path.join(G, e["rpw"]))
    templates = list(w["samples_features"].values())
    max_len = max(len(t) for t in templates)
    _, agg = orc.score_stream(mf, templates, mode=e["score_mode"])
    avg = None
    if e["avg_threshold"] != 0.0:   # WakewordComparator::run_detection :83-85: the averaged template is only scored then
        avg = np.array([orc.score_window(mf[i:i + max_len], w["avg_features"]) for i in range(len(agg))], np.float32)
    vad = e.get("vad_mode")
    got = scan_ref(agg, avg, mf.shape[0], max_len, e["threshold"], e["avg_threshold"], e.get("min_scores", 5), False,
                   vad_values_ref(mf) if vad else None, VAD_MODE_VALUE.get(vad, 0.0))

    d = orc.Detector(avg_threshold=e["avg_threshold"], threshold=e["threshold"], min_scores=e.get("min_scores", 5),
                     score_mode=e["score_mode"], vad_mode=vad)
    d.add_ref(w)
    want = []
    for i in range(0, len(s) - 479, 480):
        r = d.process_i16(s[i:i + 480])
        if r is not None:
            want.append((i // 480, r))
    assert len(want) == len(e["detections"])
    assert len(got) == len(want)
    for (frame, window, counter, avg_score, score), (chunk, r) in zip(got, want):
        assert frame // 3 + 1 == chunk and counter == r["counter"]
        assert np.float32(score) == r["score"] and score == agg[window]
        assert np.float32(avg_score) == (r["avg_score"] if avg is not None else np.float32(0))
