"""Measures the resampler kernels against the oracle and against an f64 evaluation of the same linear map (tests/resample_ref.py:
how much of the difference to the oracle is the oracle's own f32 rounding), per route: the 48 kHz FFT kernel, the matrix kernel at
48 kHz (RP_RESAMPLE_GEMM=1, read when a context first plans a rate) and the matrix kernel at the other rates.  Errors are shares of
the stream's peak."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import rustpotter_amd as ra
from oracle import rp_oracle as orc
from resample_ref import resample_f64


def signals(fs, n):
    rng = np.random.default_rng(fs)
    t = np.arange(n)
    return np.stack([rng.uniform(-0.5, 0.5, n), 0.3 * np.sin(2 * np.pi * 440.0 * t / fs) + 0.01 * rng.standard_normal(n),
                     np.where((t // 500) % 2 == 0, 0.25, -0.25), 1e-3 * rng.standard_normal(n)]).astype(np.float32)


def report(route, fs, got, pcm):
    ref64 = resample_f64(pcm, fs)
    for s in range(len(pcm)):
        ref = orc.resample_stream(pcm[s], fs)
        peak = max(float(np.abs(ref64[s]).max()), 1e-3)
        d64, d32, dor = got[s] - ref64[s], got[s] - ref, ref - ref64[s]
        print("%-7s %6d Hz signal %d: vs f64 max %.3e rms %.3e | vs oracle max %.3e rms %.3e | oracle vs f64 max %.3e   (of the peak, %.4f)" % (
            route, fs, s, np.abs(d64).max() / peak, np.sqrt((d64 * d64).mean()) / peak, np.abs(d32).max() / peak,
            np.sqrt((d32 * d32).mean()) / peak, np.abs(dor).max() / peak, peak))


routes = [("fft48", 48000)] + [("matrix", fs) for fs in (44100, 32000, 8000, 22050, 11025, 96000)]
ctx = ra.BatchContext(device=0, host_pointers=True)
for route, fs in routes:
    pcm = signals(fs, ra.resampler_frame_lengths(fs)[0] * 7)
    report(route, fs, ctx.resample(pcm, fs), pcm)
os.environ["RP_RESAMPLE_GEMM"] = "1"
gemm = ra.BatchContext(device=0, host_pointers=True)
pcm = signals(48000, 1440 * 7)
report("gemm48", 48000, gemm.resample(pcm, 48000), pcm)
