"""The bank family's live batches and whole-recording calls, pinned bit for bit to the library of the commit before the live-lane fold
(tests/golden/live_sets_pins.json names it).  The other suites hold these paths to the oracle within a tolerance; a refactor of their
kernels (the live DTW lane, the live MLP fronts, the scan frames, stream_targets_kernel) must not move a bit.

Pinned per case: every detection (stream, frame, score bits, winner's index, label), n_det per stream, and SHA-256 over the slot-score
bytes (rp_stream_batch_slot_scores; the per-window aggregate of a batch with one wakeword per stream), the logit bytes
(rp_stream_batch_logits) and the rms / gain levels where the gain normaliser is on, each over all calls in order.

S = 65: the scan kernels take a second 64-lane block, and the DTW rows straddle streams inside a wave.  Live batches are fed in calls of 1
and 6 chunks in turn (3 and 18 new frames: both row-tile builds of the live forward, partial detections carried between calls).  Banks and
audio are tests/mixed_set_cases.py's, stream s hearing row s % 10 of its audio; the rows of indices are drawn with a fixed seed, every third
stream with a slot emptied, stream 7 with none live.

Recording (on the GPU, with RP_LIB_PATH naming a library built at the parent commit):
    RP_LIB_PATH=<parent library> python tests/test_gpu_live_sets_pins.py <parent commit id>"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # recording: what tests/conftest.py gives a test run
    _tests = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [_tests, os.path.dirname(_tests)]
import mixed_set_cases as X
import model_set_cases as M

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live_sets_pins.json")
S = 65
PIECES = (1, 6)
MAX_DET = 8
N_REFS, N_MODELS = len(X.REF_LENS), len(M.MODELS)
REF_LEVELS = np.array([2e-4, float("nan"), 6e-4], np.float32)
MODEL_LEVELS = np.array([5e-4, 1e-4, float("nan"), 3e-4, float("nan"), 9e-4], np.float32)

# name: (kind, reference set size, model set size, band_size, score_mode, vad, gain normaliser, device pointers)
LIVE = {
    "bank": ("bank", 1, 0, 5, "Max", False, False, False),
    "bank_band3_median_vad": ("bank", 1, 0, 3, "Median", True, False, False),
    "bank_sets_1": ("bank_sets", 1, 0, 3, "Median", True, False, False),
    "bank_sets_3": ("bank_sets", 3, 0, 5, "Max", False, False, False),
    "bank_sets_8": ("bank_sets", 8, 0, 5, "Median", False, False, False),
    "model_bank": ("model_bank", 0, 1, 5, "Max", True, False, False),
    "model_sets_1": ("model_sets", 0, 1, 5, "Max", False, False, False),
    "model_sets_2_gain": ("model_sets", 0, 2, 5, "Max", False, True, False),
    "model_sets_8_vad": ("model_sets", 0, 8, 5, "Max", True, False, False),
    "mixed_3_2_gain": ("mixed", 3, 2, 5, "Max", False, True, False),
    "mixed_1_8_band3_median_vad": ("mixed", 1, 8, 3, "Median", True, False, False),
    "mixed_8_0": ("mixed", 8, 0, 5, "Max", False, False, False),
    "mixed_0_2": ("mixed", 0, 2, 5, "Max", False, False, False),
    "mixed_3_2_dev_bad_index": ("mixed", 3, 2, 5, "Median", False, False, True),
}
# name: (kind, reference set size, model set size, band_size, score_mode, vad)
WHOLE = {
    "detect_bank": ("bank", 1, 0, 5, "Max", False),
    "detect_bank_sets": ("bank_sets", 3, 0, 3, "Median", True),
    "detect_model_bank_sets": ("model_sets", 0, 2, 5, "Max", False),
    "detect_mixed_sets": ("mixed", 3, 2, 5, "Max", True),
    "detect_mixed_sets_8_0": ("mixed", 8, 0, 5, "Median", False),
}


def rows(n_entries, size, seed):
    """[S][size] indices into a bank of n_entries with -1 = empty: every third stream has a slot emptied, stream 7 none live, the last
    stream (alone in the scan's second block) all live"""
    if size == 0:
        return None
    r = np.random.default_rng(seed).integers(-1, n_entries, (S, size)).astype(np.int32)
    for s in range(0, S, 3):
        r[s, s % size] = -1
    r[7] = -1
    r[S - 1] = np.arange(size) % n_entries
    return r


def case_rows(name, nr, nm):
    seed = sum(map(ord, name))
    return rows(N_REFS, nr, seed), rows(N_MODELS, nm, seed + 1)


_PCM = []


def pcm():
    if not _PCM:
        _PCM.append(np.ascontiguousarray(X.pcm()[np.arange(S) % X.S]))
    return _PCM[0]


def config(ra, band, mode, vad):
    cfg = ra.DetectorConfig()
    cfg.threshold, cfg.avg_threshold, cfg.eager, cfg.min_scores = M.THRESHOLD, M.AVG_THRESHOLD, True, 2
    cfg.band_size, cfg.score_mode = band, getattr(ra.ScoreMode, mode)
    if vad:
        cfg.vad_mode = ra.VADMode.Easy
    return cfg


def make_banks(ra, c, gain):
    bank = ra.WakewordBank(c, wakewords=X.bank_wakewords())
    mbank = ra.ModelBank(c, models=[ra.Model(c, ws, bs) for ws, bs in M.bank_weights()], none_index=M.NONE_INDEX)
    if gain:
        bank.set_rms_levels(REF_LEVELS)
        mbank.set_rms_levels(MODEL_LEVELS)
    return bank, mbank


def det_rows(det, dww, dlab, n_det):
    out = []
    for s in range(S):
        for i in range(int(n_det[s])):
            d = det[s][i]
            assert d["stream"] == s
            out.append([s, int(d["frame"]), M.bits(d["score"]), int(dww[s][i]) if dww is not None else -1, int(dlab[s][i]) if dlab is not None else -1])
    return out


def run_live(ra, name):
    kind, nr, nm, band, mode, vad, gain, dev = LIVE[name]
    c = ra.BatchContext(device=0, host_pointers=not dev)
    bank, mbank = make_banks(ra, c, gain)
    cfg = config(ra, band, mode, vad)
    rr, mr = case_rows(name, nr, nm)
    kw = {}
    if gain:
        f = ra.FiltersConfig()
        f.gain_normalizer.enabled, f.gain_normalizer.min_gain, f.gain_normalizer.max_gain = True, 0.05, 8.0
        kw["per_stream_filters"] = f
    if dev:
        return run_live_dev(ra, c, bank, mbank, cfg, rr, mr)
    if kind == "bank":
        sb = ra.StreamBatch(c, None, cfg, S, max_chunks_per_call=max(PIECES), bank=bank, stream_wakeword=rr[:, 0], **kw)
    elif kind == "bank_sets":
        sb = ra.StreamBatch(c, None, cfg, S, max_chunks_per_call=max(PIECES), bank=bank, stream_wakewords=rr, **kw)
    elif kind == "model_bank":
        sb = ra.StreamBatch(c, None, cfg, S, max_chunks_per_call=max(PIECES), model_bank=mbank, stream_model=mr[:, 0], **kw)
    elif kind == "model_sets":
        sb = ra.StreamBatch(c, None, cfg, S, max_chunks_per_call=max(PIECES), model_bank=mbank, stream_models=mr, **kw)
    else:
        sb = ra.StreamBatch(c, None, cfg, S, max_chunks_per_call=max(PIECES), bank=bank, stream_wakewords=rr, model_bank=mbank, stream_models=mr, **kw)
    x = pcm()
    total = x.shape[1] // 480
    dets, n_det = [], np.zeros(S, np.int64)
    slot, logit, level = hashlib.sha256(), hashlib.sha256(), hashlib.sha256()
    at = k = 0
    while at < total:
        n = min(PIECES[k % len(PIECES)], total - at)
        k += 1
        part = np.ascontiguousarray(x[:, at * 480:(at + n) * 480])
        if kind == "bank":   # one wakeword per stream: the per-window aggregate is the call's own output
            det, nd, agg = sb.process(part, max_det=MAX_DET, want_agg=True)
            dww = dlab = None
            slot.update(agg.tobytes())
        else:
            det, dww, dlab, nd = sb.process_multi(part, max_det=MAX_DET)
        dets += det_rows(det, dww, dlab, nd)
        n_det += nd
        if kind == "bank_sets" or (kind == "mixed" and nr):
            a, v = sb.slot_scores()
            slot.update(a.tobytes()); slot.update(v.tobytes())
        if kind in ("model_bank", "model_sets") or (kind == "mixed" and nm):
            logit.update(sb.logits().tobytes())
        if gain:
            r, g = sb.levels()
            level.update(r.tobytes()); level.update(g.tobytes())
        at += n
    sb.close()
    return {"det": dets, "n_det": [int(v) for v in n_det], "slot_sha256": slot.hexdigest(), "logit_sha256": logit.hexdigest(),
            "level_sha256": level.hexdigest()}


def run_live_dev(ra, c, bank, mbank, cfg, rr, mr):
    """everything on the device; an index outside its bank is an empty slot by the kernels' own rule (the host cannot see it)"""
    import torch
    rr, mr = rr.copy(), mr.copy()
    rr[1, 0], rr[S - 1, 1], mr[2, 1], mr[S - 1, 0] = N_REFS, -9, N_MODELS + 1, 77
    dr, dm = torch.from_numpy(rr).cuda(), torch.from_numpy(mr).cuda()
    nmax = max(PIECES)
    sb = ra.StreamBatch(c, None, cfg, S, max_chunks_per_call=nmax, bank=bank, stream_wakewords=dr.data_ptr(), set_size=rr.shape[1], model_bank=mbank,
                        stream_models=dm.data_ptr(), model_set_size=mr.shape[1])
    x = torch.from_numpy(pcm()).cuda()
    total = x.shape[1] // 480
    det = torch.zeros((S, MAX_DET, np.dtype(ra.api.DET_DTYPE).itemsize), dtype=torch.uint8, device="cuda")
    dw, dl = torch.zeros((S, MAX_DET), dtype=torch.int32, device="cuda"), torch.zeros((S, MAX_DET), dtype=torch.int32, device="cuda")
    dn = torch.zeros(S, dtype=torch.int32, device="cuda")
    dets, n_det = [], np.zeros(S, np.int64)
    slot, logit = hashlib.sha256(), hashlib.sha256()
    at = k = 0
    torch.cuda.synchronize()
    while at < total:
        n = min(PIECES[k % len(PIECES)], total - at)
        k += 1
        part = x[:, at * 480:(at + n) * 480].contiguous()
        agg = torch.zeros((S, rr.shape[1], 3 * n), dtype=torch.float32, device="cuda")
        avg = torch.zeros_like(agg)
        lg = torch.zeros((S, mr.shape[1], 3 * n, mbank.label_pitch), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        sb.process_multi_dev(part.data_ptr(), 3, n, n * 480, det.data_ptr(), dw.data_ptr(), dl.data_ptr(), dn.data_ptr(), MAX_DET)
        sb.slot_scores_dev(agg.data_ptr(), avg.data_ptr())
        sb.logits_dev(lg.data_ptr())
        c.synchronize()
        d = np.frombuffer(det.cpu().numpy().tobytes(), dtype=ra.api.DET_DTYPE).reshape(S, MAX_DET)
        nd = dn.cpu().numpy()
        dets += det_rows(d, dw.cpu().numpy(), dl.cpu().numpy(), nd)
        n_det += nd
        slot.update(agg.cpu().numpy().tobytes()); slot.update(avg.cpu().numpy().tobytes())
        logit.update(lg.cpu().numpy().tobytes())
        at += n
    sb.close()
    return {"det": dets, "n_det": [int(v) for v in n_det], "slot_sha256": slot.hexdigest(), "logit_sha256": logit.hexdigest(),
            "level_sha256": hashlib.sha256().hexdigest()}


def run_whole(ra, name):
    kind, nr, nm, band, mode, vad = WHOLE[name]
    c = ra.BatchContext(device=0, host_pointers=True)
    bank, mbank = make_banks(ra, c, False)
    cfg = config(ra, band, mode, vad)
    rr, mr = case_rows(name, nr, nm)
    x = pcm()
    slot = hashlib.sha256()
    if kind == "bank":
        det, nd, agg, avg = c.batch_detect_bank(x, bank, rr[:, 0], cfg, max_det=2 * MAX_DET, want_agg=True)
        dww = dlab = None
        slot.update(agg.tobytes()); slot.update(avg.tobytes())
    elif kind == "bank_sets":
        det, dww, nd, agg, avg = c.batch_detect_bank_sets(x, bank, rr, cfg, max_det=2 * MAX_DET, want_agg=True)
        dlab = None
        slot.update(agg.tobytes()); slot.update(avg.tobytes())
    elif kind == "model_sets":
        det, dww, dlab, nd = c.batch_detect_model_bank_sets(x, mbank, mr, cfg, max_det=2 * MAX_DET)
    else:
        det, dww, dlab, nd = c.batch_detect_mixed_sets(x, bank, rr, mbank, mr, cfg, max_det=2 * MAX_DET)
    return {"det": det_rows(det, dww, dlab, nd), "n_det": [int(v) for v in nd], "slot_sha256": slot.hexdigest(),
            "logit_sha256": hashlib.sha256().hexdigest(), "level_sha256": hashlib.sha256().hexdigest()}


def run(ra, name):
    return run_live(ra, name) if name in LIVE else run_whole(ra, name)


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_pins_winners_of_both_kinds(golden):
    """a pin of empty detection lists proves nothing: references win in pinned cases and so do models, live and over whole recordings"""
    assert len(golden["parent"]) == 40 and set(golden["cases"]) == set(LIVE) | set(WHOLE)
    for names in (LIVE, WHOLE):
        ref_wins = sum(1 for n in names for d in golden["cases"][n]["det"] if names[n][0] == "mixed" and d[4] < 0)
        model_wins = sum(1 for n in names for d in golden["cases"][n]["det"] if names[n][0] == "mixed" and d[4] >= 0)
        print("references win %d detections of the mixed cases, models %d" % (ref_wins, model_wins))
        assert ref_wins >= 1 and model_wins >= 1, (ref_wins, model_wins)
    for n in list(LIVE) + list(WHOLE):
        assert golden["cases"][n]["n_det"][7] == 0, n   # the stream without a live slot


@pytest.mark.parametrize("name", list(LIVE) + list(WHOLE))
def test_pinned(ra, golden, name):
    got, want = run(ra, name), golden["cases"][name]
    print("%s: %d detections, slot %s logit %s level %s" % (name, len(got["det"]), got["slot_sha256"][:12], got["logit_sha256"][:12], got["level_sha256"][:12]))
    assert got["n_det"] == want["n_det"]
    assert got["det"] == want["det"]
    for key in ("slot_sha256", "logit_sha256", "level_sha256"):
        assert got[key] == want[key], key


if __name__ == "__main__":
    import time

    import rustpotter_amd
    assert os.environ.get("RP_LIB_PATH"), "RP_LIB_PATH: the library built at the parent commit"
    cases = {}
    for case in list(LIVE) + list(WHOLE):
        t0 = time.time()
        cases[case] = run(rustpotter_amd, case)
        print("%s: %d detections (%d with a label) in %.1f s" % (case, len(cases[case]["det"]), sum(1 for d in cases[case]["det"] if d[4] >= 0),
                                                                 time.time() - t0), flush=True)
    with open(GOLDEN, "w") as f:
        json.dump({"parent": sys.argv[1], "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
