"""scan_kernel and vad_value_kernel (rp_scan.hip) through rp_detect_scan, on rows constructed to reach what real audio never does:
equality with the thresholds, a run or a countdown that ends on the stream's last frame, a second run inside the refill gap after a
reset, eager firing exactly at min_scores, more detections than max_det, windows of one to three frames (countdown 0 and 1), the
VAD's gate opening, its 500-frame countdown running out, its 0.01 floor, its reset -- in 130 streams: two full blocks of 64 and a block
of two lanes, with the scenarios moved over lanes 0, 63, 64, 127, 128, 129 and a few inner ones from call to call.

The witness is tests/scan_ref.py (pinned to the oracle's detector by tests/test_scan_ref.py).  Frame, window, counter and n_det are
exact; score and avg_score are the kernel's inputs copied, so bit-equal.  The output block is pre-filled with 0xFF bytes: every slot
behind a stream's detections must come back zero, for quiet streams too.  For every scenario the test also asserts, from scan_ref's
side, that it does what its name says -- a mis-built row cannot pass vacuously."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import rpw_py
import simstream
from oracle import rp_oracle as orc
from scan_ref import _Vad, scan_ref, vad_values_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
S = 130
EDGE = [0, 63, 64, 127, 128, 129]
LANES = EDGE + [9, 22, 35, 48, 77, 90, 103, 116]
THR, ATHR = F32(0.5), F32(0.2)
BG, AVG_BG = F32(0.1), F32(0.3)
DET = np.dtype([("stream", "<i4"), ("frame", "<i4"), ("window", "<i4"), ("counter", "<i4"), ("avg_score", "<f4"), ("score", "<f4")])
VAD_MODE_VALUE = {1: 2.0, 2: 2.5, 3: 3.0}   # VADMode::get_value, src/config.rs:140-146


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


def config(ra, min_scores=5, eager=False, vad_mode=None):
    c = ra.DetectorConfig()
    c.threshold, c.avg_threshold, c.min_scores, c.eager, c.vad_mode = float(THR), float(ATHR), min_scores, eager, vad_mode
    return c


def raw_scan(ra, ctx, agg, avg, n_frames, max_len, cfg, max_det, mfcc=None):
    """rp_detect_scan itself, det pre-filled with 0xFF bytes and n_det with -1 -> (det [S][max_det], n_det [S])"""
    n_streams, slots = agg.shape[0], max(max_det, 0)
    det = np.full(n_streams * slots * DET.itemsize + 8, 0xFF, np.uint8)
    n_det = np.full(n_streams, -1, np.int32)
    empty = np.zeros(1, F32)        # a call without windows still passes a row pointer

    def flat(a):
        a = np.ascontiguousarray(a, F32).reshape(-1)
        return a if a.size else empty

    agg_a, avg_a, mf_a = flat(agg), None if avg is None else flat(avg), None if mfcc is None else flat(mfcc)
    c = cfg._c()
    r = ctx._L.rp_detect_scan(ctx._h, agg_a.ctypes.data, None if avg_a is None else avg_a.ctypes.data, n_streams, n_frames, max_len,
                              C.byref(c), 1 if avg_a is not None else 0, None if mf_a is None else mf_a.ctypes.data,
                              0 if mfcc is None else mfcc.shape[-1], det.ctypes.data, n_det.ctypes.data, max_det)
    if r < 0:
        raise ra.RustpotterError(ctx._L.rp_last_error().decode("utf-8", "replace"))
    return det[: n_streams * slots * DET.itemsize].view(DET).reshape(n_streams, slots), n_det


def check_against_ref(det, n_det, agg, avg, n_frames, max_len, cfg, max_det, vad_values=None):
    """every stream of a call against scan_ref (computed once per distinct row) -> {stream: scan_ref's detections}"""
    mode_value = VAD_MODE_VALUE.get(int(cfg.vad_mode or 0), 0.0)
    cache, refs = {}, {}
    for s in range(agg.shape[0]):
        key = (agg[s].tobytes(), None if avg is None else avg[s].tobytes(), None if vad_values is None else vad_values[s].tobytes())
        if key not in cache:
            cache[key] = scan_ref(agg[s], None if avg is None else avg[s], n_frames, max_len, cfg.threshold, cfg.avg_threshold,
                                  cfg.min_scores, cfg.eager, None if vad_values is None else vad_values[s], mode_value)
        ref = refs[s] = cache[key]
        assert n_det[s] == len(ref), ("n_det", s, int(n_det[s]), ref[:4])
        k = min(len(ref), max_det)
        for i in range(k):
            d, (frame, window, counter, avg_score, score) = det[s][i], ref[i]
            assert (int(d["stream"]), int(d["frame"]), int(d["window"]), int(d["counter"])) == (s, frame, window, counter), (s, i, d, ref[i])
            assert d["score"].view(np.uint32) == F32(score).view(np.uint32) and d["avg_score"].view(np.uint32) == F32(avg_score).view(np.uint32), (s, i, d, ref[i])
        assert not det[s][k:].view(np.uint8).any(), ("slots behind the detections are zero", s, k)
    return refs


# --------------------------------------------------------------------------------------------- constructed rows
class Call:
    """the shape of one call: what the row builders need to place their runs"""

    def __init__(self, max_len, n_frames, min_scores, eager=False):
        self.max_len, self.n_frames, self.min_scores, self.eager = max_len, n_frames, min_scores, eager
        self.n_win = max(0, n_frames - max_len + 1)
        self.fire = max(1, max_len // 2)      # evaluated frames from a run's last passing window to the frame that reports it
        self.run = max(min_scores, 1)         # the shortest run that can be reported
        self.full = n_frames == 400           # the rows are laid out for 400 frames; shorter calls cut them

    def rows(self):
        return np.full(self.n_win, BG, F32), np.full(self.n_win, AVG_BG, F32)

    def frame_of(self, w):
        return w + self.max_len - 1


def put(row, start, values):
    values = np.atleast_1d(np.asarray(values, F32))
    lo, hi = max(start, 0), min(start + len(values), len(row))
    if hi > lo:
        row[lo:hi] = values[lo - start:hi - start]


def b_quiet(p, rng):
    return p.rows()


def b_single(p, rng):
    a, v = p.rows()
    put(a, 10, [0.7])
    return a, v


def b_short_and_exact(p, rng):
    """a run of min_scores - 1 windows (dropped when its countdown ends) and, clear of it, a run of exactly min_scores"""
    a, v = p.rows()
    put(a, 10, [0.7] * max(p.min_scores - 1, 0))
    put(a, p.exact_start, [0.8] * p.run)
    return a, v


def b_run_to_end(p, rng):
    a, v = p.rows()
    n = p.run + 2
    put(a, p.n_win - n, [0.7] * n)
    return a, v


def b_expire_on_last_frame(p, rng):
    """the run's last window is `fire` frames before the stream's last frame: the countdown reaches 0 on frame n_frames - 1"""
    a, v = p.rows()
    put(a, p.n_win - 1 - p.fire - p.run + 1, [0.7] * p.run)
    return a, v


def b_close_runs_higher_second(p, rng):
    a, v = p.rows()
    n = p.close_len
    put(a, 20, [0.6] * n)
    put(a, 20 + n + p.fire // 2, [0.8, 0.7] + [0.8] * (n - 2))
    put(v, 20 + n + p.fire // 2, [0.25, 0.35])
    return a, v


def b_close_runs_equal(p, rng):
    a, v = p.rows()
    n = p.close_len
    put(a, 20, [0.7] * n)
    put(v, 20, [0.4])
    put(a, 20 + n + p.fire // 2, [0.7] * n)
    return a, v


def b_refill_gap(p, rng):
    """a run that is reported at frame F, and a second run that begins on frame F + 1 -- inside the frames the reset drops and the
    max_len frames the window needs to fill again -- and lasts `run` windows past the first window that is evaluated again"""
    a, v = p.rows()
    put(a, 10, [0.7] * p.run)
    F = p.frame_of(10 + p.run - 1) + p.fire
    first_again = 3 * ((F + 3) // 3 + 1)          # as a window index: the window that starts with the first frame after the refill
    start = F + 1 - (p.max_len - 1)
    put(a, start, [0.9] * (first_again + p.run - start))
    return a, v


def b_thresholds(p, rng):
    """three runs far apart: score == threshold (does not pass); score one ulp above with avg == avg_threshold (passes); the same with
    avg one ulp below avg_threshold (does not pass)"""
    a, v = p.rows()
    step = p.run + p.fire + p.max_len + 10
    above = np.nextafter(THR, F32(1))
    put(a, 10, [THR] * p.run)
    put(a, 10 + step, [above] * p.run)
    put(v, 10 + step, [ATHR] * p.run)
    put(a, 10 + 2 * step, [above] * p.run)
    put(v, 10 + 2 * step, [np.nextafter(ATHR, F32(0))] * p.run)
    return a, v


def b_six_runs(p, rng):
    a, v = p.rows()
    step = p.run + p.fire + p.max_len + 8
    for i in range(6):
        put(a, 5 + i * step, [0.6 + 0.05 * i] * p.run)
    return a, v


def b_random(density):
    def build(p, rng):
        a, v = p.rows()
        hit = rng.random(p.n_win) < density
        a[hit] = rng.choice(np.array([0.55, 0.6, 0.6, 0.7, 0.9, 0.5], F32), int(hit.sum()))
        v[:] = rng.choice(np.array([0.3, 0.2, 0.25, 0.1, 0.3, 0.3], F32), p.n_win)
        return a, v
    return build


SCENARIOS = [("quiet", b_quiet), ("single", b_single), ("short_and_exact", b_short_and_exact), ("run_to_end", b_run_to_end),
             ("expire_on_last_frame", b_expire_on_last_frame), ("close_runs_higher_second", b_close_runs_higher_second),
             ("close_runs_equal", b_close_runs_equal), ("refill_gap", b_refill_gap), ("thresholds", b_thresholds), ("six_runs", b_six_runs),
             ("random_0.002", b_random(0.002)), ("random_0.05", b_random(0.05)), ("random_0.5", b_random(0.5)), ("random_1", b_random(1.0))]
assert len(SCENARIOS) == len(LANES)


def build_call(p, rotate, seed):
    """-> agg [S][n_win], avg [S][n_win], {scenario: lane}; scenario i sits on LANES[(i + rotate) % 14], quiet streams everywhere else"""
    p.exact_start = 10 + max(p.min_scores - 1, 0) + p.fire + 10
    p.close_len = max(3, (p.min_scores + 1) // 2)
    rng = np.random.default_rng(seed)
    agg = np.full((S, p.n_win), BG, F32)
    avg = np.full((S, p.n_win), AVG_BG, F32)
    where = {}
    for i, (name, build) in enumerate(SCENARIOS):
        lane = LANES[(i + rotate) % len(LANES)]
        agg[lane], avg[lane] = build(p, rng)
        where[name] = lane
    return agg, avg, where


def check_scenarios(p, refs, where, with_avg):
    """from scan_ref's side: each scenario does what its name says (calls of 400 frames; the shorter ones cut the rows)"""
    if not p.full:
        assert p.n_win > 1 or not any(refs.values())      # no window, or one window: nothing can be reported
        return
    m, L, fire, r = p.min_scores, p.max_len, p.fire, p.run
    get = lambda name: refs[where[name]]
    assert get("quiet") == []
    if L <= 3:
        # countdown 0 or 1: it is 0 when the next frame is evaluated, so every partial is taken one frame after its window and no
        # counter ever passes 1 -- eager or not
        assert all(d[2] == 1 and d[0] == p.frame_of(d[1]) + 1 for ds in refs.values() for d in ds)
        if m > 1:
            assert not any(refs.values())
        else:
            assert [x[:3] for x in get("single")] == [(p.frame_of(10) + 1, 10, 1)]
            assert get("run_to_end") != [] and get("run_to_end")[-1][0] < p.n_frames
            assert [x[0] for x in get("expire_on_last_frame")] == [p.n_frames - 1]
            assert len(get("six_runs")) == 6 and len(get("random_1")) > 3
            step = r + fire + L + 10
            assert [x[1] for x in get("thresholds")] == ([10 + step] if with_avg else [10 + step, 10 + 2 * step])
        return
    if p.eager:
        # fires on the frame after the one whose window brought the counter to min_scores (min_scores 0: after the first passing window)
        d = get("short_and_exact")
        assert len(d) == 1 and d[0][2] == r and d[0][0] == p.frame_of(p.exact_start + r - 1) + 1, d
        return
    d = get("single")
    assert (d == [] and m > 1) or (m <= 1 and [x[:3] for x in d] == [(p.frame_of(10) + fire, 10, 1)]), d
    d = get("short_and_exact")
    assert len(d) == 1 and d[0][1] == p.exact_start and d[0][2] == r and d[0][0] == p.frame_of(p.exact_start + r - 1) + fire, d
    assert get("run_to_end") == []
    d = get("expire_on_last_frame")
    assert len(d) == 1 and d[0][0] == p.n_frames - 1 and d[0][2] == r, d
    n, second = p.close_len, 20 + p.close_len + fire // 2
    d = get("close_runs_higher_second")
    assert len(d) == 1 and d[0][1:3] == (second, 2 * n) and d[0][4] == F32(0.8) and (not with_avg or d[0][3] == F32(0.25)), d
    d = get("close_runs_equal")
    assert len(d) == 1 and d[0][1:3] == (20, 2 * n) and (not with_avg or d[0][3] == F32(0.4)), d
    if m <= 5:     # (at min_scores 50 the later runs of these rows do not fit into 400 frames)
        d = get("refill_gap")
        F = d[0][0]
        assert len(d) == 2 and d[1][1] == 3 * ((F + 3) // 3 + 1) and d[1][2] == r and d[1][4] == F32(0.9), d
        d = get("thresholds")
        step = r + fire + L + 10
        assert [x[1] for x in d] == ([10 + step] if with_avg else [10 + step, 10 + 2 * step]), d


@pytest.mark.parametrize("max_len", [1, 2, 3, 50])
def test_constructed_rows(ra, ctx, max_len):
    """max_len 1 .. 3: countdown 0 and 1; calls of max_len - 1 frames (no window), max_len frames (one window) and 400 frames; min_scores
    0, 1, 5, 50; eager off and on; with and without the averaged-template rows.  max_det 3: the dense rows overflow it in every call"""
    call = 0
    for n_frames in (max_len - 1, max_len, 400):
        for min_scores in (0, 1, 5, 50):
            for eager in (False, True):
                p = Call(max_len, n_frames, min_scores, eager)
                agg, avg, where = build_call(p, rotate=call, seed=1000 * max_len + call)
                for with_avg in (False, True):
                    cfg = config(ra, min_scores, eager)
                    det, n_det = raw_scan(ra, ctx, agg, avg if with_avg else None, n_frames, max_len, cfg, 3)
                    refs = check_against_ref(det, n_det, agg, avg if with_avg else None, n_frames, max_len, cfg, 3)
                    check_scenarios(p, refs, where, with_avg)
                call += 1


@pytest.mark.parametrize("max_det", [2, 1])
def test_more_detections_than_max_det(ra, ctx, max_det):
    """six runs, six detections, max_det 2 and 1: n_det is the true count, the first max_det are stored, and nothing else of the 0xFF
    block survives -- on the six edge lanes, with quiet streams between them"""
    p = Call(6, 400, 2)
    agg = np.full((S, p.n_win), BG, F32)
    for lane in EDGE:
        agg[lane], _ = b_six_runs(p, None)
    cfg = config(ra, 2)
    det, n_det = raw_scan(ra, ctx, agg, None, 400, 6, cfg, max_det)
    refs = check_against_ref(det, n_det, agg, None, 400, 6, cfg, max_det)
    assert all(d[2] == 2 for d in refs[0])
    assert all(len(refs[lane]) == 6 for lane in EDGE) and sum(len(r) for r in refs.values()) == 36
    assert n_det.tolist() == [6 if s in EDGE else 0 for s in range(S)]


def test_argument_checks(ra, ctx):
    agg = np.full((S, 10), BG, F32)
    cfg = config(ra)
    for max_len in (0, -1):
        with pytest.raises(ra.RustpotterError, match="max_len must be >= 1"):
            raw_scan(ra, ctx, agg, None, 10, max_len, cfg, 4)
    with pytest.raises(ra.RustpotterError, match="max_det must be >= 0"):
        raw_scan(ra, ctx, agg, None, 10, 1, cfg, -1)
    det, n_det = raw_scan(ra, ctx, agg, None, 10, 1, cfg, 4)      # the context is usable afterwards
    assert not n_det.any() and not det.view(np.uint8).any()


# --------------------------------------------------------------------------------------------- VAD
VAD_FRAMES, VAD_LEN, VAD_MIN_SCORES = 900, 20, 5
LOW, HIGH = 0.02, 1.0


def voiced_frames(env, mode_value):
    """which frames a VadDetector that is fed every frame calls voice"""
    vad = _Vad(mode_value)
    return np.array([vad.is_voice(x) for x in env], bool)


def vad_streams(mode_value):
    """-> {name: (envelope [900], agg row)}.  Runs are `run` windows long; a run `at` frame f has its first window END on frame f"""
    n_win, run = VAD_FRAMES - VAD_LEN + 1, 8

    def row(*frames, length=run, also=()):
        a = np.full(n_win, BG, F32)
        for f in frames:
            put(a, f - (VAD_LEN - 1), [0.7] * length)
        for f in also:
            put(a, f - (VAD_LEN - 1), [0.7])
        return a

    out = {}
    # silence, then speech from frame 100 on: the gate opens with the eleventh high frame
    env = np.full(VAD_FRAMES, LOW, F32); env[100:] = HIGH
    opens = int(np.flatnonzero(voiced_frames(env, mode_value))[0])
    out["gate_opens"] = (env, row(opens - 3, length=11), opens)
    # speech (30 high frames after 20 low ones), then quiet for good: the countdown of 500 frames runs out
    env = np.full(VAD_FRAMES, LOW, F32); env[20:50] = HIGH
    last = int(np.flatnonzero(voiced_frames(env, mode_value))[-1])
    assert last + 40 < VAD_FRAMES
    out["countdown_keeps"] = (env, row(last), last)          # the run's first window is the last voiced frame: the partial carries it on
    out["countdown_loses"] = (env, row(last + 1), last)      # one frame later nothing is evaluated any more
    # the three short partials (one window each, dropped after `fire` frames) during which the VAD is not fed: the countdown, and the
    # frames that leave the VAD's window, run 3 * fire = 30 frames late, so a run 25 frames behind `last` is still evaluated ...
    out["partials_not_fed"] = (env, row(last + 25, also=(200, 300, 400)), last)
    out["partials_sibling"] = (env, row(last + 25), last)    # ... and is lost without them
    # levels under the floor of 0.01: 0.015 is not `high` over a floor of 0.01 (it would be over the true minimum 0.001)
    env = np.full(VAD_FRAMES, 0.001, F32); env[100:] = 0.015
    out["under_floor"] = (env, row(300), None)
    env = np.full(VAD_FRAMES, 0.001, F32); env[100:] = 0.05
    out["over_floor"] = (env, row(300), None)
    # a detection resets the VAD: all-high frames after it never open the gate again (no low frame to compare with) ...
    env = np.full(VAD_FRAMES, LOW, F32); env[100:] = HIGH
    out["reset_closes"] = (env, row(200, 400), None)
    # ... and a new low-then-high stretch does
    env = env.copy(); env[300:320] = LOW
    out["reset_reopens"] = (env, row(200, 400), None)
    return out


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_vad(ra, ctx, mode):
    """mfcc_size 3; the frames' |coefficients| are 0.7 : 1.9 : 0.4 of the envelope (a little jittered, so that the order of the f32
    sum matters), i.e. the VAD's value of a frame is the envelope's"""
    mode_value = VAD_MODE_VALUE[mode]
    streams = vad_streams(mode_value)
    names = list(streams)
    n_win = VAD_FRAMES - VAD_LEN + 1
    rng = np.random.default_rng(7)

    def frames_of(envelope):
        jitter = np.ones((VAD_FRAMES, 3), F32)
        jitter[:, 0] += (rng.random(VAD_FRAMES) * 1e-4).astype(F32)
        jitter[:, 2] -= jitter[:, 0] - 1          # keeps 0.7 a + 1.9 b + 0.4 c close to 3: the thresholds keep their margins
        return (envelope[:, None] * np.array([0.7, -1.9, 0.4], F32) * jitter).astype(F32)

    env = np.tile(streams["gate_opens"][0], (S, 1))
    agg = np.full((S, n_win), BG, F32)
    mfcc = np.tile(frames_of(env[0]), (S, 1, 1))     # the quiet streams share one row (scan_ref runs once per distinct row)
    where = {}
    for i, name in enumerate(names):
        lane = LANES[(i + mode) % len(LANES)]
        env[lane], agg[lane] = streams[name][0], streams[name][1]
        mfcc[lane] = frames_of(env[lane])
        where[name] = lane
    values = np.stack([vad_values_ref(mfcc[s]) for s in range(S)])
    assert np.abs(values / env - 1).max() < 1e-3
    cfg = config(ra, VAD_MIN_SCORES, False, ra.VADMode(mode))
    det, n_det = raw_scan(ra, ctx, agg, None, VAD_FRAMES, VAD_LEN, cfg, 4, mfcc=mfcc)
    refs = check_against_ref(det, n_det, agg, None, VAD_FRAMES, VAD_LEN, cfg, 4, vad_values=values)
    # what the same rows give without a VAD
    plain = {name: scan_ref(agg[where[name]], None, VAD_FRAMES, VAD_LEN, THR, ATHR, VAD_MIN_SCORES, False, None, 0.0) for name in names}
    get = lambda name: refs[where[name]]
    opens = streams["gate_opens"][2]
    d = get("gate_opens")      # windows ending on frames opens - 3 .. opens + 7: only the eight from `opens` on are evaluated
    assert len(d) == 1 and d[0][2] == 8 and d[0][1] == opens - (VAD_LEN - 1) and plain["gate_opens"][0][2] == 11, d
    last = streams["countdown_keeps"][2]
    d = get("countdown_keeps")
    assert len(d) == 1 and d[0][2] == 8 and d[0][1] == last - (VAD_LEN - 1), d
    assert get("countdown_loses") == [] and len(plain["countdown_loses"]) == 1
    d = get("partials_not_fed")
    assert len(d) == 1 and d[0][2] == 8 and d[0][1] == last + 25 - (VAD_LEN - 1), d
    assert get("partials_sibling") == [] and len(plain["partials_sibling"]) == 1
    assert get("under_floor") == [] and len(plain["under_floor"]) == 1 and len(get("over_floor")) == 1
    assert len(get("reset_closes")) == 1 and len(plain["reset_closes"]) == 2 and len(get("reset_reopens")) == 2


# --------------------------------------------------------------------------------------------- the three ways to the same detections
def test_detect_paths_agree_on_130_streams(ra, ctx):
    """rolled copies of the reference's simulation stream on the edge lanes, noise everywhere else: rp_batch_detect detect-only (the
    aggregate pass's per-stream flags tell the scan which streams to run), with the score arrays requested, and rp_dtw_score_batch +
    rp_detect_scan (the scan sweeps the rows itself) give the same bytes"""
    e = json.load(open(os.path.join(simstream.GOLDEN, "expectations.json")))["simulation"]["max"]
    w = rpw_py.load_rpw(os.path.join(simstream.GOLDEN, e["rpw"]))
    base = simstream.i16_to_f32(simstream.simulation_stream_i16())
    n = (len(base) // 480) * 480
    pcm = np.empty((S, n), F32)
    for s in range(S):
        pcm[s] = np.roll(base[:n], 480 * 3 * EDGE.index(s)) if s in EDGE else orc.synth_pcm(0x5EED000000000001, s, n) * F32(0.05)
    tm = ra.Templates(ctx, list(w["samples_features"].values()), avg=w["avg_features"])
    cfg = config(ra, 5)
    det0, n0 = ctx.batch_detect(pcm, tm, cfg, max_det=4)
    det1, n1, _, _ = ctx.batch_detect(pcm, tm, cfg, max_det=4, want_scores=True)
    mf = ctx.mfcc(pcm, 5)
    _, avg, agg = ctx.dtw_scores(mf, tm, with_avg=True)
    det2, n2 = raw_scan(ra, ctx, agg, avg, mf.shape[1], tm.max_len, cfg, 4)
    assert n0.tolist() == [2 if s in EDGE else 0 for s in range(S)]
    assert np.array_equal(n0, n1) and np.array_equal(n0, n2)
    assert det0.tobytes() == det1.tobytes() and det0.tobytes() == det2.tobytes()
    assert [int(det0[s][0]["counter"]) for s in EDGE] == [21] * 6     # the golden detection, wherever the stream was rolled to
