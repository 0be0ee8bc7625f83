"""The filter kernels of rp_frontend.hip (rp_frontend_batch: decode + GainNormalizerFilter + BandPassFilter over whole streams) at every
build and row layout, bit for bit against orc.frontend_stream like the other front-end tests: no tolerance anywhere in this file.
  chunk RMS      chunk_rms_staged_kernel (default), chunk_rms_kernel vec4 arm (RP_FRONTEND_RMS=0; also what live batches launch), its
                 one-sample arm (rows not aligned to four samples)
  gain           gain_kernel with the window in LDS (window_size <= 192) and in the global ring (above)
  gain + biquad  apply_filters_lines_kernel<TIN, GAIN, BP, 64, 2> (default), <..., 128, 1> (RP_FRONTEND_TILE=128), apply_filters_kernel
                 (rows or output not aligned to four samples)"""
import numpy as np
import pytest

import child_runs
from oracle import rp_oracle as orc

pytestmark = pytest.mark.gpu

GAIN = dict(min_gain=0.2, max_gain=3.0, rms_level_ref=0.05)
BAND = dict(low_cutoff=120.0, high_cutoff=900.0)
WINDOW = 7
SILENT, HALF_SILENT, SPIKES = 5, 64, (66, 129)
SENTINEL = np.float32(-12345.0)


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def decode(raw):
    return raw if raw.dtype == np.float32 else raw.astype(np.float32) / np.float32(32767.0)


def rows(kind, S, N):
    """[S][N] input, row s the same whatever S: noise of rms 0.05 .. 0.18 (seven levels by row), except
      row SILENT       digital silence: rms 0, the gain stays 1 and the window is left alone
      row HALF_SILENT  silence over the first half
      rows SPIKES      f32: noise of 1e-3 with one sample of +-1.09 a chunk -- chunk rms 0.04975, gain round(10 * sqrt(0.05 / 0.04975)) / 10
                       == 1 exactly while samples lie outside [-1, 1]: they must pass unclamped (the comment at one() in
                       apply_filters_lines_kernel); i16: the same with full-scale spikes."""
    x = np.empty((S, N), np.float32)
    for s in range(S):
        rng = np.random.default_rng([9, s])
        if s in SPIKES:
            x[s] = rng.standard_normal(N) * 1e-3
            at = np.arange(0, N, 480) + (37 + 11 * np.arange(len(range(0, N, 480)))) % 480
            at = at[at < N]
            x[s, at] = np.where(np.arange(len(at)) % 2 == 0, 1.09, -1.09)
        else:
            x[s] = rng.standard_normal(N) * ((1500.0 + 750.0 * (s % 7)) / 32767.0)
    if S > SILENT:
        x[SILENT] = 0
    if S > HALF_SILENT:
        x[HALF_SILENT, :N // 2] = 0
    return x if kind == "f32" else np.round(np.clip(x, -1, 1) * 32767.0).astype(np.int16)


def filters(ra, gain, band):
    f = ra.FiltersConfig()
    f.gain_normalizer.enabled, f.gain_normalizer.min_gain, f.gain_normalizer.max_gain = gain, GAIN["min_gain"], GAIN["max_gain"]
    f.band_pass.enabled, f.band_pass.low_cutoff, f.band_pass.high_cutoff = band, BAND["low_cutoff"], BAND["high_cutoff"]
    return f


def oracle(x, gain, band, window=WINDOW):
    return orc.frontend_stream(decode(x), gain_normalizer=gain, window_size=window, band_pass=band, **GAIN, **BAND)


def same_as_oracle(got, raw, gain, band, streams, window=WINDOW, what=""):
    out, rms, gains = got
    for s in streams:
        ro, rr, rg = oracle(raw[s], gain, band, window)
        assert np.array_equal(bits(rms[s]), bits(rr)), (what, s, "rms")
        assert np.array_equal(bits(gains[s]), bits(rg)), (what, s, "gains")
        assert np.array_equal(bits(out[s]), bits(ro)), (what, s, "out")


# ------------------------------------------------------------------------------------------- every stream
@pytest.mark.parametrize("kind", ["i16", "f32"])
@pytest.mark.parametrize("N", [480 * 9 + 36, 480, 476], ids=["9chunks+36", "1chunk", "no-chunk"])
def test_every_stream_of_two_workgroups_and_a_partial_one(ra, ctx, N, kind):
    """130 streams = two full workgroups and two rows, both filters on, ALL streams compared (row 63 is the last of a full workgroup, 64
    the first of the next, 128 and 129 the partial one whose loads clamp the row and whose stores test it).  One chunk is 7.5 tiles for the
    two waves of apply_filters_lines_kernel<..., 64, 2>; fewer than 480 samples are no chunk at all: the output is the decoded input."""
    S = 130
    raw = rows(kind, S, N)
    got = ctx.frontend(raw, filters(ra, True, True), GAIN["rms_level_ref"], WINDOW)
    assert got[0].shape == (S, N) and got[1].shape == got[2].shape == (S, N // 480)
    same_as_oracle(got, raw, True, True, range(S))
    if N < 480:
        assert np.array_equal(bits(got[0]), bits(decode(raw)))
        return
    assert np.all(got[1][SILENT] == 0) and np.all(got[2][SILENT] == 1) and (N == 480 or got[2][HALF_SILENT][0] == 1)
    assert np.all(got[2][list(SPIKES)] == 1) and len(np.unique(got[2])) > 3
    if kind == "f32":  # the premise of rows SPIKES, and with the band-pass off the samples themselves: a gain of exactly 1 is no clamp
        assert np.abs(raw[list(SPIKES)]).max() > 1
        out, _, gains = ctx.frontend(raw, filters(ra, True, False), GAIN["rms_level_ref"], WINDOW)
        assert np.all(gains[list(SPIKES)] == 1) and np.array_equal(bits(out[list(SPIKES)]), bits(raw[list(SPIKES)]))
        same_as_oracle((out, got[1], gains), raw, True, False, range(S))


# ------------------------------------------------------------------------------------------- the gain window in global memory
LONG_S, LONG_CHUNKS = 70, 450


@pytest.fixture(scope="module")
def long_rows():
    """70 streams x 450 chunks of low-amplitude noise: a level of its own per stream, 0.012 .. 0.1 and far from its neighbours', that swings
    by a factor of two either way over 170 chunks -- the window's mean keeps moving, and most gains lie inside the clamp"""
    rng = np.random.default_rng(11)
    s, c = np.arange(LONG_S)[:, None, None], np.arange(LONG_CHUNKS)[None, :, None]
    level = (10.0 ** (-1.92 + 0.92 * ((s * 37) % LONG_S) / LONG_S + 0.3 * np.sin(2 * np.pi * c / 170.0 + s))).astype(np.float32)
    x = rng.standard_normal((LONG_S, LONG_CHUNKS, 480), dtype=np.float32) * level * np.float32(32767.0)
    return np.round(x).astype(np.int16).reshape(LONG_S, LONG_CHUNKS * 480)


@pytest.mark.parametrize("window", [192, 193, 400])
def test_gain_window_in_global_memory(ra, ctx, long_rows, window):
    """gain_kernel keeps a lane's RMS window in LDS while window_size * 256 B fits 48 KB: 192 is the last size that does, 193 and 400 run
    the ring in global memory, [S][window_size].  450 chunks: the window fills, wraps and keeps sliding.  Streams 0, 63, 64 and 69 ==
    the oracle (rms, gains, filtered samples); and the gains of ALL 70 streams == those of a second call with the streams in reversed
    order -- stream s is then lane / ring slice 69 - s, in the other workgroup for most: a slice that depends on anything but the lane's
    own stream index and window_size shows."""
    f = filters(ra, True, True)
    got = ctx.frontend(long_rows, f, GAIN["rms_level_ref"], window)
    same_as_oracle(got, long_rows, True, True, (0, 63, 64, 69), window)
    assert ((got[2] > GAIN["min_gain"]) & (got[2] < GAIN["max_gain"])).mean() > 0.9 and len(np.unique(got[2][0, window:])) > 1
    _, rms_r, gains_r = ctx.frontend(np.ascontiguousarray(long_rows[::-1]), f, GAIN["rms_level_ref"], window)
    assert np.array_equal(bits(rms_r[::-1]), bits(got[1])) and np.array_equal(bits(gains_r[::-1]), bits(got[2]))


# ------------------------------------------------------------------------------------------- the A/B builds
AB_S = (1, 64, 70)
AB_N = (480 * 1, 480 * 9 + 36, 480 * 8)
COMBOS = ((False, False), (True, False), (False, True), (True, True))


def ab_calls(ra, ctx):
    """every (S, N, input type, gain, band-pass) of the A/B test -> {name/out, name/rms, name/gains}"""
    res = {}
    for S in AB_S:
        for N in AB_N:
            for kind in ("i16", "f32"):
                raw = rows(kind, S, N)
                for gain, band in COMBOS:
                    out, rms, gains = ctx.frontend(raw, filters(ra, gain, band), GAIN["rms_level_ref"], WINDOW)
                    name = "S%d-N%d-%s-g%d-b%d" % (S, N, kind, gain, band)
                    res[name + "/out"], res[name + "/rms"], res[name + "/gains"] = out, rms, gains
    return res


CHILD = """import test_gpu_frontend_builds as t
np.savez(sys.argv[1], **t.ab_calls(ra, ctx))
"""


def test_ab_builds_give_the_default_builds_bits(ra, ctx, tmp_path):
    """RP_FRONTEND_TILE=128 (apply_filters_lines_kernel<TIN, GAIN, BP, 128, 1>: one wave on 128-sample tiles), RP_FRONTEND_RMS=0 (the vec4
    arm of chunk_rms_kernel, the kernel launch_chunk_rms runs for live batches) and both, one child each (the variables are read once per
    process).  S in {1, 64, 70} x N in {480, 480 * 9 + 36, 480 * 8} x {i16, f32} x the four (gain, band-pass) settings: out, rms and gains
    of every child == the default build's (lines<..., 64, 2>, chunk_rms_staged_kernel) bit for bit, and those == the oracle for every
    stream."""
    settings = [("tile128", {"RP_FRONTEND_TILE": "128"}), ("rms0", {"RP_FRONTEND_RMS": "0"}), ("both", {"RP_FRONTEND_TILE": "128", "RP_FRONTEND_RMS": "0"})]
    got = child_runs.run_each(tmp_path, CHILD, settings, timeout=120)
    mine = ab_calls(ra, ctx)
    assert len(mine) == 3 * len(AB_S) * len(AB_N) * 2 * len(COMBOS)
    for S in AB_S:
        for N in AB_N:
            for kind in ("i16", "f32"):
                raw = rows(kind, S, N)
                for gain, band in COMBOS:
                    name = "S%d-N%d-%s-g%d-b%d" % (S, N, kind, gain, band)
                    same_as_oracle([mine[name + "/" + k] for k in ("out", "rms", "gains")], raw, gain, band, range(S), what=name)
    for name, _ in settings:
        assert set(got[name]) == set(mine)
        for k, v in mine.items():
            assert got[name][k].shape == v.shape and np.array_equal(bits(got[name][k]), bits(v)), (name, k)


# ------------------------------------------------------------------------------------------- device pointers and pitches
@pytest.mark.parametrize("kind", ["i16", "f32"])
def test_device_pointers_and_pitches(ra, ctx, kind):
    """rp_frontend_batch on device pointers (BatchContext.frontend_dev), 70 streams of 480 * 9 + 36 samples, both filters on.  The ABI has
    a separate out_stride, so the output rows sit 8 floats apart inside a buffer of sentinels:
      pcm_stride N, N + 4   chunk_rms_staged_kernel + apply_filters_lines_kernel<..., 64, 2>
      pcm_stride N + 1      the one-sample arm of chunk_rms_kernel + apply_filters_kernel (rows not aligned to four samples)
      out_stride N + 3      the same two, chosen by the output rows (pcm_stride N)
    The padding between the input rows is NaN (f32) / the most negative value (i16) and must never reach a result; every layout == the
    packed host-pointer call bit for bit, sentinels in the output's padding and around it intact."""
    import torch
    S, N = 70, 480 * 9 + 36
    nc = N // 480
    raw = rows(kind, S, N)
    f = filters(ra, True, True)
    want = ctx.frontend(raw, f, GAIN["rms_level_ref"], WINDOW)
    same_as_oracle(want, raw, True, True, range(S))
    bad = np.float32("nan") if kind == "f32" else np.iinfo(np.int16).min
    fmt = ra.SampleFormat.F32 if kind == "f32" else ra.SampleFormat.I16
    dctx = ra.BatchContext(device=0, host_pointers=False)
    pad = 64
    for pitch, opitch in ((N, N + 8), (N + 4, N + 8), (N + 1, N + 8), (N, N + 3)):
        host = np.full((S, pitch), bad, raw.dtype)
        host[:, :N] = raw
        d_pcm = torch.from_numpy(host).cuda()
        d_out = torch.full((pad + S * opitch + pad,), float(SENTINEL), dtype=torch.float32, device="cuda")
        d_rms = torch.full((S, nc), float(SENTINEL), dtype=torch.float32, device="cuda")
        d_gains = torch.full((S, nc), float(SENTINEL), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dctx.frontend_dev(d_pcm.data_ptr(), fmt, S, N, pitch, f, GAIN["rms_level_ref"], WINDOW, d_out.data_ptr() + 4 * pad, opitch,
                          d_rms.data_ptr(), d_gains.data_ptr())
        dctx.synchronize()
        got = d_out.cpu().numpy()
        assert np.all(got[:pad] == SENTINEL) and np.all(got[-pad:] == SENTINEL), (pitch, opitch)
        block = got[pad:-pad].reshape(S, opitch)
        assert np.all(block[:, N:] == SENTINEL), (pitch, opitch)
        assert not np.isnan(block).any()
        assert np.array_equal(bits(block[:, :N]), bits(want[0])), (pitch, opitch)
        assert np.array_equal(bits(d_rms.cpu().numpy()), bits(want[1])) and np.array_equal(bits(d_gains.cpu().numpy()), bits(want[2])), (pitch, opitch)
    with pytest.raises(ra.RustpotterError, match="stride smaller than n_samples"):
        dctx.frontend_dev(d_pcm.data_ptr(), fmt, S, N, N - 1, f, GAIN["rms_level_ref"], WINDOW, d_out.data_ptr(), N)
