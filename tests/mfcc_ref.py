"""Plain f64 reference of the MFCC pipeline (src/mfcc/extractor.rs:60-198) and the comparison that tests/test_gpu_mfcc_f64.py holds the
kernel to: the kernel must be as good an f32 evaluation of the formula as the f32 oracle is.  The only f32 quantities are the ones the
reference itself keeps in f32 -- its tables, taken from the oracle and widened, the decoded input samples and the pre-emphasised samples
it stores; every transform, product and sum is f64.  tests/test_mfcc_ref.py pins the oracle to it on the CPU, on the signals below."""
import numpy as np

from oracle import rp_oracle as orc

SEED = 0x5EED000000000001

# Sample::into_f32 (src/audio/audio_types.rs): an f32 division by the type's scale
SCALE = {np.dtype(np.int8): 127.0, np.dtype(np.int16): 32767.0, np.dtype(np.int32): 2147483648.0}


def decode(raw):
    """i8 / i16 / i32 / f32 samples -> f32 the way Sample::into_f32 does"""
    raw = np.asarray(raw)
    if raw.dtype == np.float32:
        return raw
    return raw.astype(np.float32) / np.float32(SCALE[raw.dtype])


def f64_mfcc(pcm, K):
    """The reference's formula in double precision: pre-emphasis restarted every 160 samples and rounded to f32 as the reference stores it
    (extractor.rs:87-97), Hamming window (f32 table), DFT-480, |X|^2 on bins 0..239, mel bank (f32 table, no normalisation), ln(x +
    f32::MIN_POSITIVE), un-normalised DCT-II x 2 (f32 cosine table), c0 dropped; frame j = shifts j+1..j+3."""
    ham = orc.hamming_window().astype(np.float64)
    fb, _ = orc.mel_filter_bank(K)
    dct = orc.dct_table(K).astype(np.float64)
    nch = len(pcm) // 480
    x = np.asarray(pcm[: nch * 480], np.float32).astype(np.float64).reshape(-1, 160)
    pre = x.copy()
    pre[:, 1:] = x[:, 1:] - np.float64(np.float32(0.97)) * x[:, :-1]
    pre = np.float32(pre).astype(np.float64).reshape(-1)
    out = []
    for j in range(3 * nch - 3):
        fr = pre[(j + 1) * 160:(j + 4) * 160] * ham
        P = np.abs(np.fft.fft(fr)[:240]) ** 2
        lg = np.log(fb.astype(np.float64) @ P + np.finfo(np.float32).tiny)
        out.append(2 * (dct @ lg)[1:])
    return np.array(out)


def tones(rng, n):
    t = np.arange(n) / 16000.0
    return sum(np.sin(2 * np.pi * rng.uniform(50, 7900) * t + rng.uniform(0, 6.28)) for _ in range(int(rng.integers(1, 4))))


def utterance(rng, n):
    t = np.arange(n, dtype=np.float64) / 16000.0
    x = np.zeros(n)
    for _ in range(int(rng.integers(2, 6))):
        f0, f1 = rng.uniform(120, 3500, 2)
        ph = 2 * np.pi * np.cumsum(np.linspace(f0, f1, n)) / 16000.0
        env = np.interp(t, np.linspace(0, t[-1], 8), rng.uniform(0.0, 1.0, 8))
        x += rng.uniform(0.05, 0.3) * env * np.sin(ph + rng.uniform(0, 6.28))
    return x + rng.standard_normal(n) * 0.003


# ---- the signal families of tests/test_gpu_mfcc_f64.py (the same arrays on the CPU, tests/test_mfcc_ref.py, and on the device)
ROUTES = ("vector", "scalar", "i16")


def noise(first_stream, n_streams, route="vector"):
    """synth_pcm broadband noise, 60 chunks a stream.  route "scalar": two more samples a row (an odd pitch: one sample per load in the
    kernel; the tail is shorter than a chunk and reaches no frame); "i16": the same noise as 16-bit samples, decoded by the kernel."""
    assert route in ROUTES
    n = 480 * 60 + (2 if route == "scalar" else 0)
    sig = [orc.synth_pcm(SEED, first_stream + s, n) for s in range(n_streams)]
    if route == "i16":
        sig = [np.round(x * np.float32(32767.0)).astype(np.int16) for x in sig]
    return sig


def large_size_signals(route="vector"):
    return noise(0, 6, route)


def broadband_signals(route="vector"):
    return noise(40, 4, route)


def steady_tone_signals():
    rng = np.random.default_rng(2)
    return [tones(rng, 480 * 40) * 10.0 ** rng.uniform(-1.5, 0.3) for _ in range(8)]


def speech_like_signals():
    rng = np.random.default_rng(3)
    return [utterance(rng, 480 * 40) * 10.0 ** rng.uniform(-1.5, 0.3) for _ in range(8)]


def as_input(x):
    """what the kernel is handed: integer samples as they are, everything else as f32"""
    x = np.asarray(x)
    return np.ascontiguousarray(x if x.dtype in SCALE else x.astype(np.float32))


_REF = {}


def oracle_and_f64(signals, K, key=None):
    """(oracle, f64) frames of every signal, concatenated, as float64 -- both from the DECODED f32 samples.  `key` names the family:
    the pair is computed once and shared (read-only) by the tests that need it."""
    if key is not None and (key, K) in _REF:
        return _REF[(key, K)]
    ref, tru = [], []
    for x in signals:
        x = decode(as_input(x))
        ref.append(orc.mfcc_stream(x, K).astype(np.float64))
        tru.append(f64_mfcc(x, K))
    ref, tru = np.concatenate(ref), np.concatenate(tru)
    ref.setflags(write=False); tru.setflags(write=False)
    if key is not None:
        _REF[(key, K)] = (ref, tru)
    return ref, tru


def gate_scale(ref, framescale):
    """what a gate is relative to: the frame's largest coefficient (tests/test_gpu_parity.py mfcc_close_framescale) or the element"""
    return np.maximum(np.abs(ref).max(axis=1, keepdims=True), 1.0) if framescale else np.maximum(np.abs(ref), 1.0)


def compare_arrays(got, ref, tru, loose_gate, framescale):
    """kernel / oracle / f64 frames [n][K] as float64; asserts that the kernel is as good an f32 evaluation as the oracle and returns
    (largest kernel-vs-oracle error in units of the strict gate, the oracle's largest error, the kernel's largest error)."""
    assert got.shape == ref.shape == tru.shape and got.shape[0] > 100
    ek, eo = np.abs(got - tru), np.abs(ref - tru)
    # the kernel is no worse an f32 evaluation than the oracle: rms error overall and per coefficient, largest error overall
    rk, ro = np.sqrt((ek ** 2).mean(axis=0)), np.sqrt((eo ** 2).mean(axis=0))
    print("rms ratio %.3f, per coefficient %.3f, largest error %.3f (oracle %.3g, kernel %.3g)" %
          (np.sqrt((ek ** 2).mean()) / np.sqrt((eo ** 2).mean()), (rk / ro).max(), ek.max() / eo.max(), eo.max(), ek.max()))
    assert np.sqrt((ek ** 2).mean()) <= 1.15 * np.sqrt((eo ** 2).mean()), np.sqrt((ek ** 2).mean()) / np.sqrt((eo ** 2).mean())
    assert np.all(rk <= 1.4 * ro), (rk / ro).max()
    assert ek.max() <= 2.5 * eo.max(), ek.max() / eo.max()
    # the loosened gate itself -- an element beyond it must be one where the kernel is the closer of the two -- and where the strict gate
    # is exceeded the kernel stays inside the oracle's own error band
    strict = 1e-5 * np.maximum(np.abs(ref), 1.0)
    scale = gate_scale(ref, framescale)
    viol = np.abs(got - ref) > loose_gate * scale
    assert np.all(ek[viol] <= eo[viol]), float((np.abs(got - ref) / scale).max())
    beyond = np.abs(got - ref) > strict
    assert np.all(ek[beyond] <= 2.5 * np.broadcast_to(eo.max(axis=0), ek.shape)[beyond])
    return float((np.abs(got - ref) / strict).max()), float(eo.max()), float(ek.max())


def compare(ctx, signals, K, loose_gate, framescale, key=None):
    """compare_arrays with the kernel's frames of every signal (one stream a call, through ctx.mfcc: integer signals are decoded by the
    kernel, a row length that is no multiple of four takes the one-sample loads)"""
    got = np.concatenate([ctx.mfcc(as_input(x)[None, :], K)[0].astype(np.float64) for x in signals])
    ref, tru = oracle_and_f64(signals, K, key)
    return compare_arrays(got, ref, tru, loose_gate, framescale)
