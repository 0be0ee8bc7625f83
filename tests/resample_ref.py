"""Plain f64 reference of the resampler in front of the detector (rubato FftFixedInOut, src/audio/encoder.rs:72-83), vectorised over
streams with numpy: what tests/test_gpu_resample_routes.py compares the device kernels with.  The only f32 quantities are the ones
rubato itself holds in f32 -- the filter spectrum, taken from the oracle (orc.Resampler(fs).filter_spectrum()) and widened -- and the
decoded input samples; every transform, product and sum is f64.  tests/test_resample_ref.py pins it to the oracle."""
import numpy as np

from oracle import rp_oracle as orc

# Sample::into_f32 (src/audio/audio_types.rs): an f32 division by the type's scale
SCALE = {np.dtype(np.int8): 127.0, np.dtype(np.int16): 32767.0, np.dtype(np.int32): 2147483648.0}


def decode(raw):
    """i8 / i16 / i32 / f32 samples -> f32 the way Sample::into_f32 does (the table of sweep_parity.run_resample_sweep)"""
    raw = np.asarray(raw)
    if raw.dtype == np.float32:
        return raw
    return raw.astype(np.float32) / np.float32(SCALE[raw.dtype])


_SPECTRA = {}


def filter_spectrum(fs):
    """(fi, fo, filter spectrum [fi + 1] as complex128): rubato's f32 values, widened"""
    if fs not in _SPECTRA:
        r = orc.Resampler(fs)
        _SPECTRA[fs] = (r.in_len, r.out_len, r.filter_spectrum().astype(np.complex128))
    return _SPECTRA[fs]


def resample_f64(x, fs, block=512):
    """x f32 [S][n] (or [n]) at fs -> float64 [S][(n // fi) * fo] at 16 kHz; the ragged tail (n % fi samples) is dropped the way
    chunks_exact drops it.  Streams are taken `block` at a time to bound the memory of the spectra."""
    x = np.asarray(x)
    assert x.dtype == np.float32, "the reference takes the decoded f32 samples"
    if x.ndim == 1:
        x = x[None, :]
    fi, fo, h = filter_spectrum(fs)
    S, n = x.shape
    n_chunks = n // fi
    new_len = fi + 1 if fi < fo else fo
    out = np.zeros((S, n_chunks * fo), np.float64)
    if n_chunks == 0:
        return out
    for s0 in range(0, S, block):
        frames = x[s0:s0 + block, :n_chunks * fi].astype(np.float64).reshape(-1, n_chunks, fi)
        spec = np.fft.rfft(frames, 2 * fi, axis=2)[:, :, :new_len] * h[:new_len]   # zero-padded to 2*fi, filtered, truncated
        spec[:, :, 0] = spec[:, :, 0].real                                         # realfft ignores the imaginary part of bin 0
        y = np.fft.irfft(spec, 2 * fo, axis=2) * (2 * fo)                          # unnormalised inverse; bins new_len.. are zero
        o = out[s0:s0 + block].reshape(-1, n_chunks, fo)
        o[:] = y[:, :, :fo]
        o[:, 1:] += y[:, :-1, fo:]                                                 # overlap-add; silence before frame 0
    return out
