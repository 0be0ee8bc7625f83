"""Pins tests/mfcc_ref.py -- the f64 numpy statement of the MFCC pipeline that tests/test_gpu_mfcc_f64.py holds the kernel to -- to the
f32 oracle, on the CPU, for every signal family, mfcc size and input route those tests use: the oracle lies inside the gate of its family
(the gates of tests/test_gpu_parity.py and tests/sweep_parity.py run_mfcc_sweep, as they are), and the premises the device tests assert
about the oracle's own distance from the exact value hold.  Every premise held for every case when this file was written (printed
below: the oracle is 1.5e-5 .. 7e-5 from f64 on the large sizes, 1.5e-4 on steady tones), so none is dropped."""
import numpy as np
import pytest

import mfcc_ref
from oracle import rp_oracle as orc

# (family, signals, K, gate, relative to the frame's largest coefficient, the premise on the oracle's largest error or None)
CASES = [("large-%s" % r, lambda r=r: mfcc_ref.large_size_signals(r), K, 1e-5, True, 4e-6)
         for r, Ks in (("vector", (16, 23, 40, 13)), ("scalar", (16,)), ("i16", (16,))) for K in Ks]
CASES += [("broadband-%s" % r, lambda r=r: mfcc_ref.broadband_signals(r), 5, 1e-5, False, None) for r in mfcc_ref.ROUTES]
CASES += [("tones", mfcc_ref.steady_tone_signals, 5, 1e-4, False, 1e-5), ("speech", mfcc_ref.speech_like_signals, 5, 3e-5, False, None)]


@pytest.mark.parametrize("key,signals,K,gate,framescale,premise", CASES, ids=["%s-K%d" % (c[0], c[2]) for c in CASES])
def test_the_oracle_is_within_its_gate_of_f64(key, signals, K, gate, framescale, premise):
    sig = signals()
    ref, tru = mfcc_ref.oracle_and_f64(sig, K, key)
    assert ref.shape == tru.shape == (sum(3 * (len(x) // 480) - 3 for x in sig), K) and ref.shape[0] > 100
    eo = np.abs(ref - tru)
    rel = float((eo / mfcc_ref.gate_scale(ref, framescale)).max())
    print("%s K %d: oracle - f64: largest %.3g, %.3g of the gate's scale (gate %g)" % (key, K, eo.max(), rel, gate))
    assert rel <= gate
    if premise is not None:
        assert eo.max() > premise


def test_routes_feed_the_same_noise():
    """the scalar route is the vector route's samples plus a tail that reaches no frame; the i16 route is that noise to the nearest
    16-bit value, and both references are computed from what the kernel decodes"""
    v, s, i = (mfcc_ref.large_size_signals(r) for r in mfcc_ref.ROUTES)
    assert all(len(x) == 480 * 60 and x.dtype == np.float32 for x in v) and all(len(x) == 480 * 60 + 2 for x in s)
    assert all(np.array_equal(a, b[:len(a)]) for a, b in zip(v, s))
    assert np.array_equal(orc.mfcc_stream(s[0], 13), orc.mfcc_stream(v[0], 13)) and np.array_equal(mfcc_ref.f64_mfcc(s[0], 13), mfcc_ref.f64_mfcc(v[0], 13))
    assert all(x.dtype == np.int16 and len(x) == 480 * 60 for x in i)
    d = mfcc_ref.decode(i[0])
    assert d.dtype == np.float32 and np.array_equal(d, i[0].astype(np.float32) / np.float32(32767.0)) and np.abs(d - v[0]).max() <= 0.5 / 32767 + 1e-7
    assert mfcc_ref.as_input(i[0]).dtype == np.int16 and mfcc_ref.as_input(np.zeros(4)).dtype == np.float32


def test_f64_mfcc_shapes_and_framing():
    """frame j covers shifts j+1..j+3; fewer than two chunks give no frame; a tail shorter than a chunk is dropped"""
    x = orc.synth_pcm(mfcc_ref.SEED, 3, 480 * 4 + 77)
    m = mfcc_ref.f64_mfcc(x, 5)
    assert m.dtype == np.float64 and m.shape == (9, 5)
    assert mfcc_ref.f64_mfcc(x[:480], 5).shape[0] == 0 and mfcc_ref.f64_mfcc(x[:479], 5).shape[0] == 0
    assert np.array_equal(mfcc_ref.f64_mfcc(x[:480 * 4], 5), m)
    assert np.array_equal(mfcc_ref.f64_mfcc(x[480:], 5), m[3:])   # frames depend on their own three shifts only
    ref, tru = mfcc_ref.oracle_and_f64([x, x], 5, key="framing")
    assert ref.shape == (18, 5) and mfcc_ref.oracle_and_f64([], 5, key="framing")[0] is ref and not ref.flags.writeable
