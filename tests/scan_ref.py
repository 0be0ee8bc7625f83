"""The detector's state machine over one stream's precomputed window scores, in plain Python: what scan_kernel and vad_value_kernel
(rp_scan.hip) must reproduce.  Restated from the reference -- Rustpotter::process_audio / process_new_mfccs / run_detection /
is_detection_done (src/detector.rs:347-454), Rustpotter::reset (:290-302) and VadDetector (src/mfcc/vad.rs) -- with the oracle's
det_run_detection / process_new_mfccs / vad_is_voice (oracle/rp_oracle.c) as the worked example.  It walks the reference's own objects
(a frame window that fills and drains, an extractor that loses its history on reset, a partial detection that is taken) instead of the
kernel's bookkeeping (win_start / resume), so that agreeing with the kernel means something.  tests/test_scan_ref.py pins it to
orc.Detector on the golden simulation stream.

Every comparison is made on np.float32 values.

What it stands in for: one wakeword whose aggregate (and, optionally, averaged-template) score of every window is given.  A window is
the max_len frames that end at a frame; row w of `agg` / `avg` is the window that starts at frame w.  Constructed rows reach scan_kernel
only through rp_detect_scan (its sweep path; rp_batch_detect runs the same kernel behind the aggregate pass's per-stream flags).  The live
form scan_stream_kernel, the bank's scan_bank_kernel and the several-wakeword form of scan_kernel take their rows from the DTW / MLP
kernels inside one call of the ABI -- constructed rows cannot reach them -- and keep their own live == offline, bank and multi-wakeword
tests.
"""
import numpy as np

F32 = np.float32
VAD_WINDOW, VAD_VOICE_FRAMES, VAD_MIN_FLOOR = 50, 500, F32(0.01)


def vad_values_ref(mfcc):
    """[n_frames][K] -> the value VadDetector::is_voice forms of every frame: |coefficients| summed in order, in f32, over K"""
    m = np.abs(np.asarray(mfcc, F32))
    s = np.zeros(m.shape[0], F32)
    for k in range(m.shape[1]):
        s = s + m[:, k]          # f32 + f32, one coefficient at a time: the order of iter().sum()
    return s / F32(m.shape[1])


class _Vad:  # src/mfcc/vad.rs
    def __init__(self, mode_value):
        self.mode_value = F32(mode_value)
        self.reset()

    def reset(self):
        self.window = np.full(VAD_WINDOW, np.nan, F32)
        self.index = 0
        self.voice_countdown = 0

    def is_voice(self, value):
        self.window[self.index] = value
        self.index = 0 if self.index >= VAD_WINDOW - 1 else self.index + 1
        known = self.window[~np.isnan(self.window)]
        low = max(known.min(), VAD_MIN_FLOOR)
        th = F32(low * self.mode_value)
        if int(np.count_nonzero(self.window > th)) > 10:
            self.voice_countdown = VAD_VOICE_FRAMES
        if self.voice_countdown > 0:
            self.voice_countdown -= 1
            return True
        return False


def scan_ref(agg, avg, n_frames, max_len, threshold, avg_threshold, min_scores, eager, vad_values, vad_mode_value, fpf=3, label=None):
    """-> [(frame, window, counter, avg_score, score)]: the detections of one stream, `frame` the MFCC frame whose processing returned it.

    agg / avg: the stream's rows (avg None: no averaged-template test, avg_score 0); vad_values: vad_values_ref of the stream's frames or
    None (no VAD).  fpf: MFCC frames a chunk of input adds (3 for 480-sample chunks).  label: a row like agg, what each window's detection
    carries besides its scores (a model's label); a detection then has a sixth entry, the label of the window that holds its score -- the
    partial detection is replaced as a whole or only counted up (detector.rs:416-428), so it is the label of `window`."""
    agg = list(np.asarray(agg, F32))
    avg = None if avg is None else list(np.asarray(avg, F32))
    threshold, avg_threshold = F32(threshold), F32(avg_threshold)
    vad = None if vad_values is None else _Vad(vad_mode_value)
    out = []
    window_len = 0            # audio_mfcc_window.len()
    partial = None            # [window, counter, avg_score, score, label]
    countdown = 0
    # MfccExtractor: frame f is the four hops f .. f + 3 of 160 samples, a chunk brings fpf hops, so frame f comes out of chunk
    # c = (f + 3) // fpf.  A detection in chunk c drops the rest of c (find_map) and resets the extractor; it starts again with the
    # first hop of chunk c + 1, and the first frame it completes begins there: fpf * (c + 1)
    skip_until = 0
    for f in range(n_frames):
        if f < skip_until:
            continue
        # process_new_mfccs
        should_run = partial is not None or vad is None or vad.is_voice(vad_values[f])
        window_len += 1
        emitted = False
        if window_len >= max_len and should_run:
            # run_detection
            w = f - max_len + 1
            if countdown != 0:
                countdown -= 1
            if partial is not None and (countdown == 0 or (eager and partial[1] >= min_scores)):
                taken, partial = partial, None
                if taken[1] >= min_scores:
                    out.append((f, taken[0], taken[1], taken[2], taken[3]) + (() if label is None else (taken[4],)))
                    # reset()
                    window_len = 0
                    if vad is not None:
                        vad.reset()
                    skip_until = fpf * ((f + 3) // fpf + 1)
                    emitted = True
            if not emitted:
                score, avg_score = agg[w], F32(0)
                found = score > threshold
                if avg is not None:
                    avg_score = avg[w]
                    found = found and not (avg_score < avg_threshold)
                if found:
                    counter = 1 if partial is None else partial[1] + 1
                    if partial is None or partial[3] < score:
                        partial = [w, counter, avg_score, score, None if label is None else label[w]]
                    else:
                        partial[1] = counter
                    countdown = max_len // 2
        if not emitted and window_len >= max_len:
            window_len -= 1       # drain(0..1)
    return out
