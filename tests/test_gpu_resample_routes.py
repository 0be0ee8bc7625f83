"""The resampler in front of the detector (rp_resample.hip) at the shapes production uses, on every route, against a plain f64
reference (tests/resample_ref.py, pinned to the oracle by tests/test_resample_ref.py):

 a. resample48_fft_kernel with waves that carry several consecutive frames (the overlap half handed on in LDS, the prefetch chain, a
    ragged last run, a last workgroup with one live wave) -- every other resampler test has one frame per wave;
 b. every sample type, the vector load (32-bit mono) against the scalar one (the same samples as channel 0 of interleaved input), and
    the staged copy against reading in place;
 c. the device-pointer entry rp_resample_batch with every pointer / stride alignment that picks a route, padding that must stay
    untouched, nothing-to-do calls and the refusals;
 d. resample_mfma_kernel with more than one workgroup (rows and waves past the end in a block that is not the first);
 e. live batches whose calls carry runs of several frames, the previous input frame kept per stream by the run that owns the last one.

Two kinds of assertion.  EXACT: one output frame depends on its input frame and the one before only, and the FFT kernel evaluates it
the same way whatever the split, so all its routes agree bit for bit on the same decoded samples.  ACCURACY: max |got - ref| and the
rms of got - ref, as shares of the stream's peak, against resample_f64 -- per route, over uniform noise, a tone in noise, a square
wave and white noise at -60 dBFS, with type-min / type-max samples planted at frame edges.

Measured on an MI355X (worst stream of every test here; max share, rms share):
    route                          max      rms     gate (max, rms)
    FFT kernel, 48 kHz             7.2e-7   1.6e-7  1.08e-6, 2.4e-7    (a, b, c: i8 / i16 / i32 / f32, in place and staged)
    matrix kernel, 48 kHz          2.88e-6  5.1e-7  4e-6 (capped), 7.7e-7
    matrix kernel, 44.1 kHz        2.54e-6  5.0e-7  3.81e-6, 7.5e-7
    matrix kernel, 32 kHz          2.16e-6  5.2e-7  3.24e-6, 7.7e-7
    matrix kernel, 8 kHz           1.08e-6  2.1e-7  1.62e-6, 3.2e-7
    matrix kernel, 22.05 kHz       2.14e-6  4.3e-7  3.21e-6, 6.4e-7
    matrix kernel, 11.025 kHz      1.41e-6  2.9e-7  2.12e-6, 4.3e-7
    matrix kernel, 96 kHz          3.46e-6  6.6e-7  5.19e-6, 9.9e-7
(the FFT kernel's error is a quarter of the matrix kernel's: log-depth butterflies against a 2 880-term f32 sum; the oracle itself lies
1.8e-7 from f64, tests/test_resample_ref.py.)
The gates below are the larger of 1.5 x those and the reference's f32-output floor (half an ulp at the peak, 6e-8; rms 3.5e-8), and
never looser than the gate the suite applies against the oracle, 4e-6 * max(1, sqrt(fi / 1440)) (test_gpu_parity._audio_scale_close,
sweep_parity.run_resample_sweep)."""
import os

import numpy as np
import pytest

import rpw_py
import simstream
from resample_ref import decode, resample_f64

pytestmark = pytest.mark.gpu
G = simstream.GOLDEN

FI = {48000: 1440, 44100: 1323, 32000: 960, 8000: 240, 22050: 882, 11025: 441, 96000: 2880}


def oracle_gate(fs):
    return 4e-6 * max(1.0, (FI[fs] / 1440.0) ** 0.5)


# route -> (max share, rms share) measured (see the table above); the gate is derived in gate()
MEASURED = {
    "fft48": (7.21e-7, 1.63e-7),
    "gemm48": (2.88e-6, 5.12e-7),
    44100: (2.54e-6, 4.99e-7),
    32000: (2.16e-6, 5.16e-7),
    8000: (1.08e-6, 2.10e-7),
    22050: (2.14e-6, 4.28e-7),
    11025: (1.41e-6, 2.87e-7),
    96000: (3.46e-6, 6.61e-7),
}
FLOOR_MAX, FLOOR_RMS = 2.0 ** -24, 2.0 ** -24 / 3.0 ** 0.5


def gate(route):
    fs = 48000 if route in ("fft48", "gemm48") else route
    mx, rms = MEASURED[route]
    return min(max(1.5 * mx, FLOOR_MAX), oracle_gate(fs)), min(max(1.5 * rms, FLOOR_RMS), oracle_gate(fs))


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


# ------------------------------------------------------------------------------------------------------------ inputs and checks
def make_raw(S, n, fs, dtype, seed):
    """[S][n] samples of `dtype`, every stream its own: stream s is of kind s % 4 -- uniform noise, a tone (its own pitch) in noise, a
    square wave (its own period and phase), white noise at -60 dBFS.  Every seventh stream and the last one carry the type's minimum
    and maximum (f32: -1 and 1) at the first and last sample of every frame, alternating."""
    rng = np.random.default_rng([seed, S, n, fs])
    fi = FI[fs]
    x = np.empty((S, n), np.float32)
    t = np.arange(n, dtype=np.float64)
    kind = np.arange(S) % 4
    i0, i1, i2, i3 = (np.flatnonzero(kind == k) for k in range(4))
    x[i0] = rng.random((len(i0), n), dtype=np.float32) - np.float32(0.5)
    f = rng.uniform(50.0, 7000.0, len(i1))
    x[i1] = (0.3 * np.sin(2 * np.pi * f[:, None] * t[None, :] / fs)).astype(np.float32) + \
        np.float32(0.01) * rng.standard_normal((len(i1), n), dtype=np.float32)
    p, ofs = rng.integers(50, 900, len(i2)), rng.integers(0, 900, len(i2))
    x[i2] = np.where(((np.arange(n)[None, :] + ofs[:, None]) // p[:, None]) % 2 == 0, np.float32(0.25), np.float32(-0.25))
    x[i3] = np.float32(1e-3) * rng.standard_normal((len(i3), n), dtype=np.float32)
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        raw, lo, hi = x, -1.0, 1.0
    else:
        info = np.iinfo(dtype)
        lo, hi = info.min, info.max
        raw = np.clip(np.round(x.astype(np.float64) * hi), lo, hi).astype(dtype)
    planted = sorted(set(range(0, S, 7)) | {S - 1})
    first, last = np.arange(0, (n // fi) * fi, fi), np.arange(fi - 1, (n // fi) * fi, fi)
    for s in planted:
        raw[s, first[0::2]], raw[s, first[1::2]] = lo, hi
        raw[s, last[0::2]], raw[s, last[1::2]] = hi, lo
    return raw


def interleave(raw, ch):
    """raw as channel 0 of ch interleaved channels; the others carry the samples in reverse (never read: reencode_to_mono)"""
    if ch == 1:
        return raw
    inter = np.empty(raw.shape + (ch,), raw.dtype)
    inter[:, :, 0] = raw
    inter[:, :, 1:] = raw[:, ::-1, None]
    return inter.reshape(raw.shape[0], -1)


def shares(got, ref):
    """(max |got - ref|, rms of got - ref) as shares of the stream's peak, the worst stream of each"""
    d = got.astype(np.float64) - ref
    peak = np.maximum(np.abs(ref).max(axis=1), 1e-3)
    return float((np.abs(d).max(axis=1) / peak).max()), float((np.sqrt((d * d).mean(axis=1)) / peak).max())


def check_accuracy(route, got, ref, what):
    assert got.shape == ref.shape and got.dtype == np.float32 and np.isfinite(got).all(), what
    mx, rms = shares(got, ref)
    gmx, grms = gate(route)
    print("%s [%s]: max %.3g rms %.3g of the peak (gates %.3g, %.3g)" % (what, route, mx, rms, gmx, grms))
    assert mx <= gmx and rms <= grms, "%s [%s]: max %.3g rms %.3g of the peak, gates %.3g / %.3g" % (what, route, mx, rms, gmx, grms)


def fft48_split(S, n_chunks):
    """(n_seg, seg_len) of launch_resample48_t: runs of seg_len consecutive frames, one wave each"""
    n_seg = min(n_chunks, 1 if S >= 8192 else -(-8192 // S))
    seg_len = -(-n_chunks // n_seg)
    return -(-n_chunks // seg_len), seg_len


def spread(S, k=16):
    """k streams over the batch: the first, the last, both sides of workgroup boundaries (four waves a workgroup) and of the middle"""
    want = [0, 1, 3, 4, 5, 7, 8, S // 3, S // 2 - 1, S // 2, S // 2 + 1, (2 * S) // 3, S - 5, S - 4, S - 2, S - 1]
    return sorted({s for s in want if 0 <= s < S})[:k]


# ------------------------------------------------------------------------------------------- a. long runs in resample48_fft_kernel
LONG = [  # S, frames, sample type, channels, (n_seg, seg_len)
    (8192, 2, np.int16, 1, (1, 2)),      # one run of two frames a stream
    (8193, 2, np.int16, 1, (1, 2)),      # ... and a last workgroup with one live wave
    (4096, 3, np.float32, 1, (2, 2)),    # runs 2 + 1
    (2731, 7, np.int16, 2, (3, 3)),      # runs 3 + 3 + 1, 8 193 waves
    (1, 8193, np.float32, 1, (4097, 2)),  # 4 097 runs, the last of one frame
    (1, 1, np.float32, 1, (1, 1)),
    (5, 1, np.int16, 1, (1, 1)),
]


@pytest.mark.parametrize("S,frames,dtype,ch,split", LONG, ids=["%dx%d" % (c[0], c[1]) for c in LONG])
def test_long_runs_match_f64_and_the_single_frame_split(ra, ctx, S, frames, dtype, ch, split):
    """a. Every stream against resample_f64; 16 streams spread over the batch bit for bit against the same streams resampled on their
    own (so few that every wave gets one frame).  The one long stream: 16 five-frame windows of it instead."""
    assert fft48_split(S, frames) == split
    raw = make_raw(S, frames * 1440, 48000, dtype, seed=1)
    inter = interleave(raw, ch)
    got = ctx.resample(inter, 48000, channels=ch)
    check_accuracy("fft48", got, resample_f64(decode(raw), 48000), "S %d x %d frames %s %d ch" % (S, frames, np.dtype(dtype).name, ch))
    if S > 1 or frames < 5:
        pick = spread(S)
        assert fft48_split(len(pick), frames)[1] == 1
        alone = ctx.resample(np.ascontiguousarray(inter[pick]), 48000, channels=ch)
        assert np.array_equal(alone, got[pick])
    else:
        starts = [0, 1, 2, 3, 1000, 1001, 4094, 4095, 4096, 4097, 6001, 6002, frames - 8, frames - 7, frames - 6, frames - 5]
        assert fft48_split(len(starts), 5)[1] == 1
        win = ctx.resample(np.stack([raw[0, f0 * 1440:(f0 + 5) * 1440] for f0 in starts]), 48000)
        for i, f0 in enumerate(starts):   # a window's first frame starts from silence, the stream's from frame f0 - 1
            skip = 0 if f0 == 0 else 480
            assert np.array_equal(win[i, skip:], got[0, f0 * 480 + skip:(f0 + 5) * 480])


# ------------------------------------------------------------------------------------------- b. sample types and the vector load
@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.int32, np.float32], ids=lambda d: np.dtype(d).name)
def test_sample_types_vector_and_scalar_loads(ra, ctx, dtype):
    """b. 4 096 streams x 3 frames (runs 2 + 1): mono (i32 / f32: the four-sample vector load), the same samples as channel 0 of 2- and
    3-channel input (the scalar load) and mono with a ragged tail (rows no longer 16-byte multiples: staged into f32 with a history
    frame in front) -- bit for bit one result, within the gate of f64."""
    S, frames = 4096, 3
    assert fft48_split(S, frames) == (2, 2)
    raw = make_raw(S, frames * 1440, 48000, dtype, seed=2)
    mono = ctx.resample(raw, 48000)
    check_accuracy("fft48", mono, resample_f64(decode(raw), 48000), "S %d x %d frames %s" % (S, frames, np.dtype(dtype).name))
    for ch in (2, 3):
        assert np.array_equal(ctx.resample(interleave(raw, ch), 48000, channels=ch), mono), "%d channels" % ch
    tail = np.full((S, 3), np.nan if np.dtype(dtype) == np.float32 else np.iinfo(dtype).min, dtype)
    ragged = np.concatenate([raw, tail], axis=1)
    assert (ragged.shape[1] * ragged.itemsize) % 16 != 0
    assert np.array_equal(ctx.resample(ragged, 48000), mono), "staged"


# ------------------------------------------------------------------------------------------- c. routes by pointer and stride
SENTINEL = np.float32(-7777.0)


class DevCase:
    """S x frames (+ a ragged tail of 8 samples) at 48 kHz on the device, rows `stride` apart behind `offset` elements; everything the
    call must not read is NaN (f32) or the type's extremes (i16); the output is S + 2 rows of sentinels"""

    def __init__(self, raw, tail, stride_pad, offset, out_pad, out_offset):
        import torch
        S, n_real = raw.shape
        self.S, self.n, self.n_out = S, n_real + tail, (n_real // 1440) * 480
        self.stride, self.out_stride, self.out_offset = self.n + stride_pad, self.n_out + out_pad, out_offset
        junk = np.nan if raw.dtype == np.float32 else np.iinfo(raw.dtype).max
        host = np.full(offset + (S + 1) * self.stride, junk, raw.dtype)
        if raw.dtype != np.float32:
            host[1::2] = np.iinfo(raw.dtype).min
        rows = host[offset:offset + S * self.stride].reshape(S, self.stride)
        rows[:, :n_real] = raw
        self.pcm = torch.from_numpy(host).cuda()
        self.out = torch.full((out_offset + (S + 2) * self.out_stride,), float(SENTINEL), dtype=torch.float32, device="cuda")
        self.pcm_ptr = self.pcm.data_ptr() + offset * raw.itemsize
        self.out_ptr = self.out.data_ptr() + out_offset * 4
        self.fmt = 3 if raw.dtype == np.float32 else 1
        assert self.pcm.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def run(self, dctx, S=None, n=None):
        dctx.resample_dev(self.pcm_ptr, self.fmt, 1, 48000, self.S if S is None else S, self.n if n is None else n, self.stride,
                          self.out_ptr, self.out_stride)
        dctx.synchronize()
        flat = self.out.cpu().numpy()
        assert np.all(flat[:self.out_offset] == SENTINEL), "in front of the output"
        rows = flat[self.out_offset:].reshape(self.S + 2, self.out_stride)
        return rows

    def result(self, dctx):
        rows = self.run(dctx)
        assert np.all(rows[:self.S, self.n_out:] == SENTINEL), "padding columns"
        assert np.all(rows[self.S:] == SENTINEL), "rows beyond S"
        got = np.ascontiguousarray(rows[:self.S, :self.n_out])
        assert np.isfinite(got).all() and not np.any(got == SENTINEL)
        return got


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=lambda d: np.dtype(d).name)
def test_device_pointer_routes(ra, dtype):
    """c. rp_resample_batch on device pointers, 64 streams x 5 frames + 8 ragged samples.  A 16-byte-aligned input with rows a multiple
    of 16 bytes apart is read in place; an input one element off, or rows 16-byte multiples apart no longer, is staged; both stay on the
    FFT kernel and equal the base bit for bit.  An odd out_stride, or an output one float off, falls to resample_mfma_kernel<30>: within
    the gate of f64 (and not the FFT kernel's bits).  Nothing outside [S][n_out] is written, nothing outside the frames is read."""
    dctx = ra.BatchContext(device=0, host_pointers=False)
    S, frames, tail = 64, 5, 8
    raw = make_raw(S, frames * 1440, 48000, dtype, seed=3)
    ref = resample_f64(decode(raw), 48000)
    eb = raw.itemsize
    assert ((frames * 1440 + tail) * eb) % 16 == 0
    base = DevCase(raw, tail, 0, 0, 0, 0).result(dctx)
    check_accuracy("fft48", base, ref, "device pointers, in place, %s" % raw.dtype.name)
    fft_variants = {"pcm one element off": (0, 1, 0, 0), "row pitch not a multiple of 16 bytes": (1, 0, 0, 0),
                    "both pitches padded by 8": (8, 0, 8, 0), "one element off and both pitches padded": (8, 1, 8, 0)}
    assert ((frames * 1440 + tail + 1) * eb) % 16 != 0
    for name, (sp, off, op, ooff) in fft_variants.items():
        assert np.array_equal(DevCase(raw, tail, sp, off, op, ooff).result(dctx), base), name
    for name, (sp, off, op, ooff) in {"out_stride = n_out + 1": (0, 0, 1, 0), "out one float off": (0, 0, 0, 1),
                                      "out one float off, padded input": (8, 1, 2, 1)}.items():
        got = DevCase(raw, tail, sp, off, op, ooff).result(dctx)
        check_accuracy("gemm48", got, ref, "device pointers, %s, %s" % (name, raw.dtype.name))
        assert not np.array_equal(got, base), "%s: expected the matrix kernel's rounding, not the FFT kernel's" % name
    # nothing to do: fewer samples than a frame, no streams -- 0 and the output untouched
    for kw in ({"n": 1439}, {"S": 0}):
        case = DevCase(raw, tail, 0, 0, 0, 0)
        assert np.all(case.run(dctx, **kw) == SENTINEL), kw
    # refusals
    case = DevCase(raw[:2], tail, 0, 0, 0, 0)
    n, n_out = case.n, case.n_out
    for args, msg in (((case.pcm_ptr, case.fmt, 0, 48000, 2, n, n, case.out_ptr, n_out), "Unsupported channel count"),
                      ((case.pcm_ptr, case.fmt, 1, 48000, 2, n, n - 1, case.out_ptr, n_out), "pcm_stride smaller than n_samples \\* channels"),
                      ((case.pcm_ptr, case.fmt, 2, 48000, 2, n, 2 * n - 1, case.out_ptr, n_out), "pcm_stride smaller than n_samples \\* channels"),
                      ((case.pcm_ptr, case.fmt, 1, 48000, 2, n, n, case.out_ptr, n_out - 1), "out_stride smaller than the resampled length")):
        with pytest.raises(ra.RustpotterError, match=msg):
            dctx.resample_dev(*args)
    dctx.synchronize()
    assert np.all(case.out.cpu().numpy() == SENTINEL)


# ------------------------------------------------------------------------------------------- d. the matrix kernel beyond one workgroup
@pytest.mark.parametrize("S,frames", [(13, 5), (16, 8)], ids=["65units", "128units"])
@pytest.mark.parametrize("fs", [44100, 32000, 8000, 22050, 11025, 96000])
def test_matrix_kernel_beyond_one_workgroup(ra, ctx, fs, S, frames):
    """d. resample_mfma_kernel takes 64 (stream, frame) units a workgroup.  65 units: a second workgroup with one live row, fifteen rows
    past the end in its first wave and three whole waves past the end; 128 units: two full workgroups.  All streams against f64."""
    fi = FI[fs]
    assert ra.resampler_frame_lengths(fs)[0] == fi
    raw = make_raw(S, frames * fi + 5, fs, np.float32, seed=4)
    got = ctx.resample(raw, fs)
    check_accuracy(fs, got, resample_f64(raw, fs), "%d Hz, %d units" % (fs, S * frames))


# ------------------------------------------------------------------------------------------- e. live batches with long runs
def test_live_batch_long_runs_equal_resample_then_offline(ra, ctx):
    """e. 1 366 live 48 kHz i16 streams, up to 8 frames a call: the calls of 8 frames run as four runs of two frames a stream (of 3 and 5:
    one frame a wave), the overlap seeded from the previous input frame `prev`, the last frame kept by the run that owns it.  Every
    call's detections and aggregate scores == rp_resample_batch over the whole recording, then rp_batch_detect, bit for bit; that
    whole-recording pass (runs of eleven frames) is itself held to f64 on 16 streams."""
    S, calls = 1366, [8, 3, 8, 5, 8, 3, 8, 5, 3, 5, 8]
    assert fft48_split(S, 8) == (4, 2) and fft48_split(S, 3)[1] == 1 and fft48_split(S, 5)[1] == 1
    w = rpw_py.load_rpw(os.path.join(G, "oye_casa_real.rpw"))
    x48, sr, _ = rpw_py.read_wav(os.path.join(G, "oye_casa_real_1.wav"))
    assert sr == 48000
    # the recording the templates were built from, twice: a window is as long as the recording (168 frames = 56 input frames), so the
    # first score exists at input frame 56 and an eager detector reports in the last call, one of 8 frames
    n = sum(calls) * 1440
    base = np.round(np.clip(np.concatenate([x48, x48])[:n] * 2.0, -1.0, 1.0) * 32767.0).astype(np.int16)
    assert len(base) == n
    rng = np.random.default_rng(6)
    rolls = rng.integers(0, 5, S)
    rolls[0] = 0
    streams = np.stack([np.roll(base, 1440 * int(r)) // (1 + s % 3) for s, r in enumerate(rolls)]).astype(np.int16)
    cfg = ra.DetectorConfig()
    cfg.threshold, cfg.avg_threshold, cfg.min_scores, cfg.eager = 0.47, 0.3, 2, True
    tm = ra.Templates(ctx, list(w["samples_features"].values()), avg=w["avg_features"])
    mono16 = ctx.resample(streams, 48000)        # six runs of eleven frames a stream
    assert fft48_split(S, sum(calls)) == (6, 11)
    pick = spread(S)
    check_accuracy("fft48", mono16[pick], resample_f64(decode(streams[pick]), 48000), "the whole recording, %d streams" % len(pick))
    det, n_det, _, agg = ctx.batch_detect(mono16, tm, cfg, want_scores=True)
    print("offline: %d detections in %d of %d streams" % (int(n_det.sum()), int((n_det > 0).sum()), S))
    assert n_det.sum() >= S // 2 and n_det[0] >= 1
    sb = ra.StreamBatch(ctx, tm, cfg, S, max_chunks_per_call=8, sample_rate=48000)
    assert sb.samples_per_chunk == 1440
    got = [[] for _ in range(S)]
    done = compared = 0
    for nc in calls:
        d, nd, a = sb.process(streams[:, done * 1440:(done + nc) * 1440], want_agg=True)
        assert a.shape == (S, 3 * nc)
        wi = 3 * done - 3 + np.arange(3 * nc) - tm.max_len + 1
        ok = (wi >= 0) & (wi < agg.shape[1])
        assert np.array_equal(a[:, ok].view(np.uint32), agg[:, wi[ok]].view(np.uint32)), "aggregate scores of the call at frame %d" % done
        compared += int(ok.sum())
        for si in np.flatnonzero(nd):
            got[si] += [_det_tuple(d[si][j]) for j in range(nd[si])]
        done += nc
    assert compared == agg.shape[1]
    assert got == [[_det_tuple(det[si][j]) for j in range(n_det[si])] for si in range(S)]


def _det_tuple(d):
    return (int(d["frame"]), int(d["window"]), int(d["counter"]), float(d["score"]), float(d["avg_score"]))
