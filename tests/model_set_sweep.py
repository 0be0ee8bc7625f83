"""Randomised cases for model sets (test infrastructure for tests/test_gpu_model_set_sweeps.py and tests/test_model_set_sweep_cases.py): random
rows of sets over the bank of tests/model_set_cases.py, random detector configs and bursts of coloured noise, through
rp_batch_detect_model_bank_sets (family "whole") and a live batch over model sets fed in random pieces (family "live"), each against ONE
oracle detector per stream with add_model per live slot in slot order.  The bar is sweep_parity's for models: events exact (chunk,
counter, winner and label), scores within 1e-4 with floor 1e-3 (sweep_parity._model_same).  A case may be set aside only by the oracle's own
verdict -- its events move under thresholds scaled by 1 -+ 1e-4 (sweep_parity.BANK_MARGIN) --, and none of the committed cases is: the seeds
below were chosen on the CPU from the oracle alone (tests/test_model_set_sweep_cases.py asserts it)."""
import numpy as np

import model_set_cases as M
import nn_decide_ref as R
import sweep_parity as sp

FAMILIES = ("whole", "live")
# family -> (seed, cases)
# (with these seeds every case fires, 31 and 19 detections, both eager settings occur and 7 and 7 non-empty sets stay silent)
SUITE = {"whole": (8, 4), "live": (8, 4)}


def make_case(family, seed, k):
    rng = np.random.default_rng([seed, k, FAMILIES.index(family)])
    S, set_size = int(rng.integers(5, 9)), int(rng.integers(2, 5))
    rows = np.full((S, set_size), -1, np.int32)
    for s in range(S):
        n_live = int(rng.integers(0 if s else 1, set_size + 1))
        for j in rng.choice(set_size, n_live, replace=False):
            rows[s, j] = int(rng.integers(0, len(M.MODELS)))   # duplicates and twins as they fall
    n_chunks = int(rng.integers(100, 134))
    pcm = np.stack([R.moving_audio(int(rng.integers(0, 1000)), int(rng.integers(30, 121)), n_chunks) for _ in range(S)]).astype(np.float32)
    cfg = {"threshold": float(rng.uniform(0.45, 0.7)), "avg_threshold": float(rng.choice([0.0, 0.3])), "min_scores": int(rng.integers(1, 4)),
           "eager": bool(rng.integers(0, 2))}
    pieces = [int(x) for x in rng.integers(1, 12, 8)]
    return {"family": family, "S": S, "set_size": set_size, "rows": rows, "pcm": pcm, "n_chunks": n_chunks, "cfg": cfg, "pieces": pieces}


def oracle_model(i, ws, bs):
    """model i with label names that say who won: "m<bank index>:<label index>" """
    m = M.model_dict(i, ws, bs)
    m["labels"] = ["none" if j == M.MODELS[i][3] else "m%d:%d" % (i, j) for j in range(M.MODELS[i][2])]
    return m


def oracle_events(case, scale=1.0):
    """-> per stream [(chunk, counter, "m<model>:<label>", score, avg_score)]"""
    from oracle import rp_oracle as orc
    weights, c = M.bank_weights(), case["cfg"]
    out = []
    for s, row in enumerate(case["rows"]):
        live = [int(mi) for mi in row if mi >= 0]
        if not live:
            out.append([])
            continue
        d = orc.Detector(avg_threshold=c["avg_threshold"] * scale, threshold=c["threshold"] * scale, min_scores=c["min_scores"], eager=c["eager"])
        for mi in live:
            d.add_model(oracle_model(mi, *weights[mi]))
        ev = []
        for k in range(case["n_chunks"]):
            r = d.process_f32(case["pcm"][s, k * 480:(k + 1) * 480])
            if r is not None:
                ev.append((k, int(r["counter"]), r["name"], float(r["score"]), float(r["avg_score"])))
        out.append(ev)
    return out


def set_aside(case):
    """the oracle's own events move under thresholds scaled by 1 -+ BANK_MARGIN: the case decides nothing"""
    base = [[e[:3] for e in ev] for ev in oracle_events(case)]
    return any([[e[:3] for e in ev] for ev in oracle_events(case, 1.0 + sign * sp.BANK_MARGIN)] != base for sign in (-1.0, 1.0))


def device_events(ra, ctx, bank, case):
    c = case["cfg"]
    cfg = ra.DetectorConfig()
    cfg.threshold, cfg.avg_threshold, cfg.min_scores, cfg.eager = c["threshold"], c["avg_threshold"], c["min_scores"], c["eager"]
    S = case["S"]
    out = [[] for _ in range(S)]

    def take(det, dmod, dlab, n_det):
        for s in range(S):
            for i in range(n_det[s]):
                d = det[s][i]
                out[s].append((int(d["frame"]) // 3 + 1, int(d["counter"]), "m%d:%d" % (dmod[s][i], dlab[s][i]), float(d["score"]), float(d["avg_score"])))
    if case["family"] == "whole":
        take(*ctx.batch_detect_model_bank_sets(case["pcm"], bank, case["rows"], cfg, max_det=32))
        return out
    sb = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=11, model_bank=bank, stream_models=case["rows"])
    k = i = 0
    while k < case["n_chunks"]:
        n = min(case["pieces"][i % len(case["pieces"])], case["n_chunks"] - k)
        i += 1
        take(*sb.process_multi(np.ascontiguousarray(case["pcm"][:, k * 480:(k + n) * 480]), max_det=12))
        k += n
    sb.close()
    return out


def run_case(ra, ctx, bank, family, k):
    case = make_case(family, SUITE[family][0], k)
    want, got = oracle_events(case), device_events(ra, ctx, bank, case)
    for s in range(case["S"]):
        sp._model_same("model sets %s case %d" % (family, k), s, got[s], want[s])
    return sum(len(w) for w in want)
