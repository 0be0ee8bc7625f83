"""Pins tests/resample_ref.py -- the f64 numpy statement of rubato's FftFixedInOut unit that the device resampler is compared with
(tests/test_gpu_resample_routes.py) -- to the oracle's frame-by-frame resampler.  The two differ only by the oracle rounding its
spectra and its output to f32 where realfft stores Complex<f32> / f32.

Measured (seven rates x three signals x 7 frames + a ragged tail): max |ref64 - oracle| = 1.76e-7 of the stream's peak (48 kHz, the
square wave; every rate lies between 1.4e-7 and 1.8e-7).  The bound is 4e-7, twice that."""
import numpy as np
import pytest

from oracle import rp_oracle as orc
from resample_ref import decode, resample_f64

RATES = [48000, 44100, 32000, 8000, 22050, 11025, 96000]


def signals(fs, fi, n):
    """the three signals of test_resample_batch_matches_oracle"""
    rng = np.random.default_rng(fs)
    t = np.arange(n)
    return np.stack([rng.uniform(-0.5, 0.5, n), 0.3 * np.sin(2 * np.pi * 440.0 * t / fs) + 0.01 * rng.standard_normal(n),
                     np.where((t // 500) % 2 == 0, 0.25, -0.25)]).astype(np.float32)


@pytest.mark.parametrize("fs", RATES)
def test_resample_f64_equals_the_oracle(fs):
    r = orc.Resampler(fs)
    fi, fo = r.in_len, r.out_len
    pcm = signals(fs, fi, fi * 7 + 123)
    ref = resample_f64(pcm, fs)
    assert ref.dtype == np.float64 and ref.shape == (3, 7 * fo)
    for s in range(3):
        want = orc.resample_stream(pcm[s], fs)
        assert want.shape == ref[s].shape
        err = float(np.abs(ref[s] - want).max()) / float(np.abs(want).max())
        print("fs %d stream %d: max |ref64 - oracle| = %.3g of the peak" % (fs, s, err))
        assert err <= 4e-7


def test_resample_f64_shapes_and_edges():
    """one stream as a vector, fewer samples than a frame, the stream blocks and the history of frame 0"""
    fi, fo = 1440, 480
    x = signals(48000, fi, fi * 3 + 7)
    whole = resample_f64(x, 48000)
    assert resample_f64(x[0], 48000).shape == (1, 3 * fo) and np.array_equal(resample_f64(x[0], 48000)[0], whole[0])
    assert resample_f64(x[:, :fi - 1], 48000).shape == (3, 0) and resample_f64(x[:0], 48000).shape == (0, 3 * fo)
    assert np.array_equal(resample_f64(x, 48000, block=2), whole)
    # a frame's output depends on that frame and the one before it only
    assert np.array_equal(resample_f64(x[:, fi:], 48000)[:, fo:], whole[:, 2 * fo:])
    assert np.abs(resample_f64(x[:, fi:], 48000)[:, :fo] - whole[:, fo:2 * fo]).max() > 1e-3
    with pytest.raises(AssertionError):
        resample_f64(x.astype(np.float64), 48000)


def test_decode_is_sample_into_f32():
    for dt, scale in ((np.int8, 127.0), (np.int16, 32767.0), (np.int32, 2147483648.0)):
        info = np.iinfo(dt)
        raw = np.array([info.min, info.max, 0, 1, -1, info.max // 3], dt)
        got = decode(raw)
        assert got.dtype == np.float32 and np.array_equal(got, raw.astype(np.float32) / np.float32(scale))
    assert decode(np.array([np.iinfo(np.int16).min], np.int16))[0] < -1.0 and decode(np.array([127], np.int8))[0] == 1.0
    f = np.array([0.25, -3.0], np.float32)
    assert decode(f) is f
