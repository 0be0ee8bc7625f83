"""mfcc_kernel beyond one tile per wave, at every build and row layout.

A wave of mfcc_kernel walks (stream, tile) pairs grid-stride and carries `s` and `tile` forward by stride_s = wave_stride / tiles_per_stream
and stride_t = wave_stride % tiles_per_stream (rp_mfcc.hip, the `wt += wave_stride` block); a wrong carry puts one stream's frames
into another stream's rows.  The instrument needs no tolerance: the same rows computed by the same build in a launch in which no wave takes
a second tile must be equal bit for bit, and that small-launch side is held to the oracle under the gates of tests/test_gpu_parity.py
(element-wise 1e-5 * max(|ref|, 1) up to mfcc_size 5, 1e-5 of the frame's largest coefficient above) on synth_pcm noise."""
import numpy as np
import pytest

import child_runs
import mfcc_ref
from oracle import rp_oracle as orc
from test_gpu_parity import mfcc_close, mfcc_close_framescale

pytestmark = pytest.mark.gpu

SEED = mfcc_ref.SEED
DTYPES = {"i8": np.int8, "i16": np.int16, "i32": np.int32}


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


def within_oracle_gate(got, ref, K):
    return mfcc_close_framescale(got, ref) and (K > 5 or mfcc_close(got, ref))


# ------------------------------------------------------------------------------------------- the walk at the default cap
@pytest.mark.parametrize("K", [5, 16])
def test_walk_at_the_default_cap(ctx, K):
    """600 streams of 12 chunks: 33 frames = 9 tiles a stream, the last one ragged (one frame), 5 400 wave-tiles = 1 350 workgroups
    against the cap of 1 024: wave_stride 4 096, stride_s 455, stride_t 1, and the first 1 304 waves take a second tile.  Every frame
    of the one call == the same streams 100 at a call (900 wave-tiles: no wave takes a second one), bit for bit; the sliced side is
    held to the oracle for every stream.  mfcc_kernel<true, 6 | 17, float>."""
    S, N = 600, 480 * 12
    pcm = ctx.synth_pcm(SEED, 0, S, N)
    whole = ctx.mfcc(pcm, K)
    sliced = np.concatenate([ctx.mfcc(pcm[s0:s0 + 100], K) for s0 in range(0, S, 100)])
    assert whole.shape == sliced.shape == (S, 33, K)
    if whole.tobytes() != sliced.tobytes():
        bad = np.flatnonzero((whole != sliced).any(axis=(1, 2)))
        raise AssertionError("streams %s... differ between one call and slices of 100" % bad[:8])
    for s in range(S):
        assert within_oracle_gate(sliced[s], orc.mfcc_stream(pcm[s], K), K), s


# ------------------------------------------------------------------------------------------- the walk with a forced cap
CAPS = (1, 3, 5)           # workgroups: wave_stride 4, 12, 20
WALK_S = (1, 2, 7)
WALK_CHUNKS = (2, 3, 4, 5, 10)   # frames 3, 6, 9, 12, 27: tiles 1, 2, 3, 3, 7; n_frames % 4 = 3, 2, 1, 0, 3
WALK_K = (5, 13, 2)        # the sparse K1T = 6 and 14 builds and the runtime-K one
LIVE_CALLS = (1, 2, 3, 5, 1, 2, 3, 5)   # chunks per live call: 3, 6, 9, 15 new frames = 1, 2, 3, 4 tiles, every last one ragged


def walk_input(kind, s, n):
    """stream s of the forced-cap calls: synth_pcm noise as f32, or the same noise as 16-bit samples"""
    x = orc.synth_pcm(SEED, 100 + s, n)
    return x if kind == "f32" else np.round(x * np.float32(32767.0)).astype(np.int16)


def forced_cap_calls(ctx):
    """every (input type, S, chunks, row length, K) of the forced-cap test through ctx.mfcc -> {name: frames}; run by the children under a
    cap and by the parent without one.  A row length of chunks * 480 + 2 is an odd pitch for either type: mfcc_kernel<false, 0, TIN>."""
    out = {}
    for kind in ("f32", "i16"):
        for S in WALK_S:
            for chunks in WALK_CHUNKS:
                for extra in (0, 2):
                    pcm = np.stack([walk_input(kind, s, chunks * 480 + extra) for s in range(S)])
                    for K in WALK_K:
                        out["%s-S%d-c%d-x%d-K%d" % (kind, S, chunks, extra, K)] = ctx.mfcc(pcm, K)
    return out


def live_templates():
    return orc.synth_templates(SEED, 2, 10, 5)


def live_config(ra):
    cfg = ra.RustpotterConfig.default().detector
    cfg.avg_threshold, cfg.threshold, cfg.min_scores = 0.0, 0.2, 1
    return cfg


def live_pcm(ctx):
    return ctx.synth_pcm(SEED, 200, 7, 480 * sum(LIVE_CALLS))


def live_aggregates(ra, ctx):
    """seven live streams fed LIVE_CALLS chunks a call -> the calls' aggregates side by side [7][3 * chunks]: mfcc_kernel<true, 6, float,
    true>, the history form"""
    pcm = live_pcm(ctx)
    sb = ra.StreamBatch(ctx, ra.Templates(ctx, live_templates()), live_config(ra), 7, max_chunks_per_call=max(LIVE_CALLS))
    parts, c = [], 0
    for n in LIVE_CALLS:
        parts.append(sb.process(pcm[:, c * 480:(c + n) * 480], want_agg=True)[2])
        c += n
    return np.concatenate(parts, axis=1)


CHILD = """import test_gpu_mfcc_walk as w
out = w.forced_cap_calls(ctx)
out["live"] = w.live_aggregates(ra, ctx)
np.savez(sys.argv[1], **out)
"""


def test_walk_with_a_forced_cap(ra, ctx, tmp_path):
    """RP_MFCC_BLOCKS = RP_MFCC_HS_BLOCKS = 1, 3, 5 workgroups (read once per process: one child each), so that waves take up to thirteen
    tiles of launches small enough to compare everywhere.  S in {1, 2, 7} x chunks in {2, 3, 4, 5, 10} x mfcc_size in {5, 13, 2} x
    {f32, i16} x {rows of whole chunks, two samples more}: (wave_stride, tiles per stream) = {4, 12, 20} x {1, 2, 3, 7}, that is
    stride_t = 0 with stride_s > 0 (tiles 1 and 2; tiles 3 at 12), stride_s = 0 (tiles 7 at 4) and neither zero (tiles 3 at 4 and 20, tiles
    7 at 12 and 20); all four residues of n_frames % 4.  Builds: mfcc_kernel<true, 6 | 14 | 0, float | int16_t> and <false, 0, float |
    int16_t>.  Each child's frames == the parent's at the default cap (no wave takes a second tile there), bit for bit; the parent's are
    held to the oracle for every stream.
    Live form (mfcc_kernel<true, 6, float, true>, cap RP_MFCC_HS_BLOCKS): seven streams fed 1, 2, 3, 5 chunks a call; (wave_stride, tiles)
    = {4, 12, 20} x {1, 2, 3, 4}, stride_t != 0 at (4, 3) and (20, 3), every call's last tile ragged.  The calls' aggregates side by side
    == batch_detect(want_scores=True) over the whole streams, bit for bit -- the equality test_stream_batch_many_streams_synthetic
    asserts at tiles_per_stream 2."""
    got = child_runs.run_each(tmp_path, CHILD, [("cap%d" % c, {"RP_MFCC_BLOCKS": str(c), "RP_MFCC_HS_BLOCKS": str(c)}) for c in CAPS], timeout=120)
    mine = forced_cap_calls(ctx)
    assert len(mine) == 2 * len(WALK_S) * len(WALK_CHUNKS) * 2 * len(WALK_K)
    # the parent's own results against the oracle, every stream (the two extra samples of a longer row reach no frame)
    for name, frames in mine.items():
        kind, S, chunks, extra, K = name.split("-")
        S, chunks, K = int(S[1:]), int(chunks[1:]), int(K[1:])
        assert frames.shape == (S, 3 * chunks - 3, K), name
        for s in range(S):
            ref = orc.mfcc_stream(mfcc_ref.decode(walk_input(kind, s, chunks * 480)), K)
            assert within_oracle_gate(frames[s], ref, K), (name, s)
    n_win = 3 * sum(LIVE_CALLS) - 3 - 10 + 1
    _, _, _, agg = ctx.batch_detect(live_pcm(ctx), ra.Templates(ctx, live_templates()), live_config(ra), want_scores=True)
    assert agg.shape == (7, n_win) and np.abs(agg).max() > 0
    for cap in CAPS:
        child = got["cap%d" % cap]
        assert set(child) == set(mine) | {"live"}
        for name, frames in mine.items():
            assert child[name].shape == frames.shape and child[name].tobytes() == frames.tobytes(), (cap, name)
        # column k of the calls side by side is the window that ends at new frame k: window k - 12 of the whole stream
        live = child["live"]
        assert live.shape == (7, 3 * sum(LIVE_CALLS)) and live[:, 12:].tobytes() == agg.tobytes(), cap


# ------------------------------------------------------------------------------------------- pitch, alignment and what is written
SENTINEL = np.float32(-12345.0)


@pytest.mark.parametrize("kind", ["f32", "i16"])
@pytest.mark.parametrize("K", [5, 16, 7])
def test_row_pitch_alignment_and_what_is_written(ra, ctx, K, kind):
    """rp_mfcc_batch / rp_mfcc_batch_fmt on device pointers: 5 rows of N = 480 * 7 + 123 samples inside a larger buffer.  N % 4 == 3, so the
    launcher's rule (rows and base aligned to four samples: 16-byte loads, else one sample per load) gives
      pitch N + 1, N + 5                                  -> mfcc_kernel<true, K1T, TIN>  (K1T 6 / 17 / 0 for mfcc_size 5 / 16 / 7)
      pitch N, N + 4, N + 64                              -> mfcc_kernel<false, 0, TIN>   (the pitch forces it)
      pitch N + 1 and N + 4 with the base one element on  -> mfcc_kernel<false, 0, TIN>   (the base forces it, with either pitch).
    The padding between the rows and the 123 samples behind a row's last chunk (chunks_exact's remainder: they reach no frame) are NaN
    (f32) / the most negative value (i16); the output is the middle of a larger buffer of sentinels.  Every layout == the packed
    host-pointer call of the same build bit for bit (vector: the rows cut to 480 * 7 samples; scalar: N samples, the tail included), no NaN
    in it, sentinels intact.
    The two builds must agree bit for bit as well: with -ffp-contract=off both decode a sample with the same SampleIn<TIN>::cvt, both
    form y = c - 0.97f * p as a product and a difference (p = 0.f at the start of a shift in both), everything after the staged samples
    is the same code, and the sparse mel passes of K1T 6 / 17 accumulate the dense pass's terms in its order less those whose weight is an
    exact +0 (fmaf(P, 0, acc) == acc for the finite P of finite input).
    Read bounds are argued from the code and not tested -- a load outside the allocation cannot be observed without provoking a fault:
    the vector loads of a tile are capped at the last whole group of the row by `lim` (rp_mfcc.hip fetch: room >= 4 because a tile
    starts at least one frame before the end of the row), the history form clamps through group_pos (g + 3 <= last), the scalar loads
    through g <= last, and g - 1 >= 160 for every tile."""
    import torch
    S, N, chunks = 5, 480 * 7 + 123, 7
    nf = 3 * chunks - 3
    raw = np.stack([walk_input(kind, 300 + s, N) for s in range(S)])
    dec = mfcc_ref.decode(raw)
    bad = np.float32("nan") if kind == "f32" else np.iinfo(np.int16).min
    raw[:, chunks * 480:] = bad
    vec_ref = ctx.mfcc(np.ascontiguousarray(raw[:, :chunks * 480]), K)
    sca_ref = ctx.mfcc(raw, K)
    assert vec_ref.shape == (S, nf, K) and not np.isnan(sca_ref).any()
    assert vec_ref.tobytes() == sca_ref.tobytes()
    for s in range(S):
        assert within_oracle_gate(vec_ref[s], orc.mfcc_stream(dec[s], K), K)
    dctx = ra.BatchContext(device=0, host_pointers=False)
    group = 4 * raw.itemsize
    pad = 64
    for pitch, off in ((N, 0), (N + 1, 0), (N + 5, 0), (N + 4, 0), (N + 64, 0), (N + 4, 1), (N + 1, 1)):
        host = np.full(off + S * pitch + 8, bad, raw.dtype)
        for s in range(S):
            host[off + s * pitch: off + s * pitch + N] = raw[s]
        d_pcm = torch.from_numpy(host).cuda()
        d_out = torch.full((pad + S * nf * K + pad,), float(SENTINEL), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        pcm_ptr, out_ptr = d_pcm.data_ptr() + off * raw.itemsize, d_out.data_ptr() + pad * 4
        vector = pcm_ptr % group == 0 and pitch % 4 == 0
        assert vector == ((pitch, off) in ((N + 1, 0), (N + 5, 0)))
        if kind == "f32":
            dctx.mfcc_dev(pcm_ptr, S, N, pitch, K, out_ptr)
        else:
            dctx.mfcc_dev_fmt(pcm_ptr, ra.SampleFormat.I16, S, N, pitch, K, out_ptr)
        dctx.synchronize()
        got = d_out.cpu().numpy()
        assert np.all(got[:pad] == SENTINEL) and np.all(got[-pad:] == SENTINEL), (pitch, off)
        frames = got[pad:-pad].reshape(S, nf, K)
        assert not np.isnan(frames).any() and not np.any(frames == SENTINEL), (pitch, off)
        assert frames.tobytes() == (vec_ref if vector else sca_ref).tobytes(), (pitch, off)
    d_out = torch.full((S * nf * K,), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(ra.RustpotterError, match="pcm_stride smaller than n_samples"):
        dctx.mfcc_dev_fmt(d_pcm.data_ptr(), ra.SampleFormat.F32 if kind == "f32" else ra.SampleFormat.I16, S, N, N - 1, K, d_out.data_ptr())
    dctx.synchronize()
    assert np.all(d_out.cpu().numpy() == SENTINEL)


# ------------------------------------------------------------------------------------------- builds x sample types
@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("K", [5, 13, 16, 7, 1, 63])
def test_integer_samples_at_every_build(ctx, K, name):
    """`v as f32 / T::MAX as f32` inside the kernel == decoding first, bit for bit, at every build: mfcc_kernel<true, 6 | 14 | 17 | 0, TIN>
    (rows of 480 * 6 samples) and <false, 0, TIN> (two samples more) for TIN = int8_t, int16_t, int32_t -- the assertion
    test_mfcc_integer_samples_decoded_on_device makes at mfcc_size 5, the extreme sample values in the first positions.  mfcc_size 63 is
    the largest the tables take: it must also agree with the oracle."""
    dtype = DTYPES[name]
    info = np.iinfo(dtype)
    rng = np.random.default_rng(4)
    for n in (480 * 6, 480 * 6 + 2):
        raw = rng.integers(info.min, info.max, size=(3, n), dtype=dtype, endpoint=True)
        raw[0, :5] = [info.min, info.max, 0, -1, 1]
        dec = mfcc_ref.decode(raw)
        got = ctx.mfcc(raw, K)
        assert got.shape == (3, 15, K) and np.array_equal(got, ctx.mfcc(dec, K))
        if K == 63:
            for s in range(3):
                assert mfcc_close_framescale(got[s], orc.mfcc_stream(dec[s], K))


@pytest.mark.parametrize("K", [64, 0])
def test_mfcc_size_outside_the_tables_is_refused(ra, ctx, K):
    with pytest.raises(ra.RustpotterError, match="mfcc_size out of the supported range 1..63"):
        ctx.mfcc(np.zeros((3, 480 * 6), np.float32), K)


@pytest.mark.parametrize("K", [13, 16])
def test_silence_is_bitwise_constant_across_streams_and_time(ctx, K):
    """test_mfcc_silence_is_bitwise_constant (one stream, mfcc_size 5) for three streams at the K1T = 14 and 17 builds"""
    got = ctx.mfcc(np.zeros((3, 480 * 12), np.float32), K)
    assert got.shape == (3, 33, K) and np.all(got == got[0, 0]) and np.isfinite(got).all()
    assert mfcc_close_framescale(got[0], orc.mfcc_stream(np.zeros(480 * 12, np.float32), K))
