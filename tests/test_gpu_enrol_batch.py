"""rp_wakeword_ref_build_batch: many wakeword references built in one call (one MFCC launch over all samples, normalisation and
DTW-aligned averaging on the device) against rp_wakeword_ref_build, one call per wakeword (MFCC per sample, normalisation and
averaging on the host): the .rpw bytes must be the same."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import rpw_py
import simstream

pytestmark = pytest.mark.gpu

G = simstream.GOLDEN


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


def read(name):
    with open(os.path.join(G, name), "rb") as f:
        return f.read()


def single(ctx, ww, mfcc_size, from_files=True):
    name, samples, thr, athr = ww
    return ctx.build_wakeword_ref(name, samples, mfcc_size, threshold=thr, avg_threshold=athr, from_files=from_files)


@pytest.mark.parametrize("from_files", [True, False])
def test_golden_wakewords_in_one_call(ctx, from_files):
    """The reference's three recorded wakewords (16 kHz i16 x 5, x 3, 48 kHz f32 x 6), one with a threshold, one with an avg_threshold,
    one with neither.  Also pins that mfcc_kernel gives a stream the same bits alone and in a padded batch."""
    wakewords = [
        ("oye casa", {w: read(w) for w in ["oye_casa_g_%d.wav" % i for i in range(1, 6)]}, 0.5, None),
        ("alexa", {w: read(w) for w in ["alexa.wav", "alexa2.wav", "alexa3.wav"]}, None, 0.2),
        ("oye casa real", {w: read(w) for w in ["oye_casa_real_%d.wav" % i for i in range(1, 7)]}, None, None),
    ]
    got = ctx.build_wakeword_refs(wakewords, 5, from_files=from_files)
    assert len(got) == 3
    for g, ww in zip(got, wakewords):
        assert g == single(ctx, ww, 5, from_files), ww[0]


def wav_bytes(x, rate, kind):
    """x: float samples in [-1, 1) -> a mono wav: kind 8 / 16 / 32 = PCM of that width (8-bit is unsigned in the file), 'f' = IEEE f32"""
    if kind == 8:
        data, tag, bits = (np.clip(np.round(x * 127), -128, 127).astype(np.int16) + 128).astype(np.uint8).tobytes(), 1, 8
    elif kind == 16:
        data, tag, bits = np.clip(np.round(x * 32767), -32768, 32767).astype("<i2").tobytes(), 1, 16
    elif kind == 32:
        data, tag, bits = np.clip(np.round(x.astype(np.float64) * 2147483647), -2147483648, 2147483647).astype("<i4").tobytes(), 1, 32
    else:
        data, tag, bits = x.astype("<f4").tobytes(), 3, 32
    fmt = struct.pack("<HHIIHH", tag, 1, rate, rate * bits // 8, bits // 8, bits)
    return b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + \
        b"data" + struct.pack("<I", len(data)) + data


def synth_wav(rng, seconds=None, rate=None, kind=None):
    rate = rate or int(rng.choice([16000, 16000, 16000, 48000, 8000]))
    kind = kind or [8, 16, 32, "f"][int(rng.integers(0, 4))]
    n = int((seconds or rng.uniform(0.4, 1.2)) * rate)
    t = np.arange(n) / rate
    x = 0.3 * np.sin(2 * np.pi * rng.uniform(150, 900) * t + rng.uniform(0, 6)) * np.sin(np.pi * t / t[-1]) ** 2 + 0.05 * rng.standard_normal(n)
    return wav_bytes(x.astype(np.float32), rate, kind)


def synth_wakewords(seed, W):
    rng = np.random.default_rng(seed)
    out = []
    for w in range(W):
        n = int(rng.integers(1, 7))
        samples = {"w%d_s%d.wav" % (w, i): synth_wav(rng) for i in range(n)}
        thr = None if rng.random() < 0.5 else float(np.float32(rng.uniform(0.3, 0.7)))
        athr = None if rng.random() < 0.5 else float(np.float32(rng.uniform(0.1, 0.3)))
        out.append(["wakeword %d" % w, samples, thr, athr])
    return rng, out


def test_synthetic_call(ra, ctx, tmp_path):
    """40 wakewords of 1..6 wavs (0.4-1.2 s; 8 / 16 / 32-bit PCM and f32; 16, 48 and 8 kHz): a single sample (avg_features null), two
    samples of one length (the name decides the fold order), and -- below the dict level, where a name can repeat -- a repeated sample name."""
    rng, wakewords = synth_wakewords(11, 40)
    wakewords[3][1] = {"only.wav": synth_wav(rng)}
    wakewords[5][1] = {"b.wav": synth_wav(rng, 0.9, 16000, 16), "a.wav": synth_wav(rng, 0.9, 16000, "f"), "c.wav": synth_wav(rng, 0.6, 48000, 16)}
    wakewords = [tuple(w) for w in wakewords]
    assert sorted({len(w[1]) for w in wakewords}) == [1, 2, 3, 4, 5, 6]
    got = ctx.build_wakeword_refs(wakewords, 13, from_files=True)
    for g, ww in zip(got, wakewords):
        assert g == single(ctx, ww, 13), ww[0]
    p = tmp_path / "w.rpw"
    p.write_bytes(got[3])
    assert rpw_py.load_rpw(str(p))["avg_features"] is None
    p.write_bytes(got[5])
    built = rpw_py.load_rpw(str(p))
    assert list(built["samples_features"]) == ["b.wav", "a.wav", "c.wav"] and built["mfcc_size"] == 13
    assert built["samples_features"]["a.wav"].shape == built["samples_features"]["b.wav"].shape == built["avg_features"].shape
    rp = ra.Rustpotter.new(ra.RustpotterConfig.default())
    rp.add_wakeword_from_buffer("w", got[5])

    # a repeated sample name (HashMap::insert replaces the earlier sample, in its place) needs the C arrays
    L = ctx._L
    first, second, third = synth_wav(rng, 0.7, 16000, 16), synth_wav(rng, 1.0, 48000, "f"), synth_wav(rng, 0.5, 16000, 8)
    names, bufs = [b"x.wav", b"y.wav", b"x.wav"], [first, second, third]

    def c_arrays(names, bufs):
        return (C.c_char_p * len(names))(*names), (C.c_char_p * len(bufs))(*bufs), (C.c_size_t * len(bufs))(*[len(b) for b in bufs])
    out, out_len = C.c_void_p(), C.c_size_t()
    cn, cb, cl = c_arrays(names, bufs)
    assert L.rp_wakeword_ref_build(ctx._h, b"rep", None, None, 3, cn, cb, cl, 5, 0, C.byref(out), C.byref(out_len)) == 0
    want = C.string_at(out, out_len.value)
    L.rp_buffer_free(out)
    # ... in the middle of a call of three wakewords
    other = wakewords[7]
    all_names = [k.encode() for k in other[1]] + names + [k.encode() for k in other[1]]
    all_bufs = list(other[1].values()) + bufs + list(other[1].values())
    cn, cb, cl = c_arrays(all_names, all_bufs)
    wn = (C.c_char_p * 3)(other[0].encode(), b"rep", other[0].encode())
    counts = (C.c_size_t * 3)(len(other[1]), 3, len(other[1]))
    outs, lens = (C.c_void_p * 3)(), (C.c_size_t * 3)()
    assert L.rp_wakeword_ref_build_batch(ctx._h, 3, wn, None, None, counts, cn, cb, cl, 5, 0, outs, lens) == 0
    res = [C.string_at(outs[i], lens[i]) for i in range(3)]
    for i in range(3):
        L.rp_buffer_free(outs[i])
    assert res[1] == want and res[0] == res[2] == ctx.build_wakeword_ref(other[0], other[1], 5, from_files=False)
    p.write_bytes(res[1])
    assert list(rpw_py.load_rpw(str(p))["samples_features"]) == ["x.wav", "y.wav"]


def test_errors(ra, ctx):
    """A wakeword the single call refuses fails the whole call with the single call's text behind the wakeword's index and name; nothing
    is handed out; the context goes on working."""
    _, wakewords = synth_wakewords(12, 20)
    wakewords = [tuple(w) for w in wakewords]
    good = ctx.build_wakeword_refs(wakewords[:4], 5)
    broken = dict(wakewords[17][1])
    k = next(iter(broken))
    broken[k] = broken[k][:30]   # cut inside the fmt chunk
    bad17 = (wakewords[17][0], broken, None, None)
    with pytest.raises(ra.RustpotterError) as e1:
        single(ctx, bad17, 5)
    with pytest.raises(ra.RustpotterError) as e2:
        ctx.build_wakeword_refs(wakewords[:17] + [bad17] + wakewords[18:], 5)
    assert str(e2.value) == "wakeword 17 (%s): %s" % (bad17[0], e1.value) and len(str(e1.value)) > 0
    with pytest.raises(ra.RustpotterError) as e3:
        ctx.build_wakeword_refs(wakewords[:2] + [("empty", {}, None, None)] + wakewords[3:5], 5)
    assert str(e3.value) == "wakeword 2 (empty): Can not create an empty wakeword"
    assert ctx.build_wakeword_refs([], 5) == []
    assert ctx.build_wakeword_refs(wakewords[:4], 5) == good
    # the C level: every out_rpw entry is NULL after a failure (they held something else before)
    L = ctx._L
    ws = [wakewords[0], bad17, wakewords[1]]
    names = (C.c_char_p * 3)(*[w[0].encode() for w in ws])
    counts = (C.c_size_t * 3)(*[len(w[1]) for w in ws])
    sn = [k.encode() for w in ws for k in w[1]]
    sb = [v for w in ws for v in w[1].values()]
    cn, cb, cl = (C.c_char_p * len(sn))(*sn), (C.c_char_p * len(sb))(*sb), (C.c_size_t * len(sb))(*[len(b) for b in sb])
    outs, lens = (C.c_void_p * 3)(0xdead0, 0xdead0, 0xdead0), (C.c_size_t * 3)(7, 7, 7)
    assert L.rp_wakeword_ref_build_batch(ctx._h, 3, names, None, None, counts, cn, cb, cl, 5, 1, outs, lens) == -1
    assert [outs[i] for i in range(3)] == [None, None, None] and [lens[i] for i in range(3)] == [0, 0, 0]
    assert L.rp_last_error().decode().startswith("wakeword 1 (%s): " % bad17[0])
