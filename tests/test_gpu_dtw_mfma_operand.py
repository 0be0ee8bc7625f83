"""dtw_mfma_kernel's window operand (rustpotter_amd/csrc/rp_dtw_mfma.hip): a lane builds the WHOLE frame of its window for one
column of a column pair and the two lane halves exchange their k-halves, where both halves used to build every column.  The change is one of
instruction count only: scores, the Max folded into the kernel and the list of pairs handed to dtw_ref_kernel must be the bits of the build
before it.  tests/golden/dtw_mfma_operand.npz holds the inputs and what the library of the commit before the change answered on an MI355X
(`python tests/test_gpu_dtw_mfma_operand.py --record` with RP_LIB_PATH naming that library wrote it), in both matrix arithmetics, at the
smallest shapes at which the column pairs can go wrong: the guarded first block alone (L = 12), odd lengths whose last pair holds a column
nobody uses (13, 17, 25), whole blocks (24, 16), four template slots (16, 17), bands 3 and 4, 3 streams x 45 windows (tiles straddle streams,
the last tile is partial), a live-stream batch (frames from global memory) and, at L = 24 and 25, a window of zero frames and one frame
beyond the norm range -- the range test looks two columns past a window's end and not three, at either parity of L."""
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dtw_mfma_operand.npz")
SEED = 0x5EED000000000077
ARITHMETICS = ["f32_matrix", "fast_split"]
S, N_WIN = 3, 45

# name: (band, L, T, special frames)
STAGED = {
    "L12_T8": (5, 12, 8, False),
    "L13_T8": (5, 13, 8, False),
    "L24_T6": (5, 24, 6, True),
    "L25_T8": (5, 25, 8, True),
    "L16_T3": (5, 16, 3, False),
    "L17_T4": (5, 17, 4, False),
    "band3_L13_T5": (3, 13, 5, False),
    "band4_L24_T7": (4, 24, 7, False),
}
LIVE = ("live_L13_T8", 13, 8, 2, 30)   # name, L, T, chunks per call (six new windows per stream and call), chunks


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _inputs(name):
    from oracle import rp_oracle as orc
    band, L, T, special = STAGED[name]
    n_frames = N_WIN + L - 1
    templates = np.stack(orc.synth_templates(SEED + 7 * L + T, T, L, 5))
    n = 480 * (n_frames // 3 + 2)
    mf = np.stack([orc.mfcc_stream(orc.synth_pcm(SEED, 31 * L + s, n), 5)[:n_frames] for s in range(S)]).astype(np.float32)
    if special:
        mf[0, 10:10 + L] = mf[0, 10]    # window 10 of stream 0: every centred frame is the zero vector (the guard)
        mf[1, 40] *= np.float32(1e17)   # one frame beyond the norm range: windows 40 - L - 1 .. 40 see it, the first two only ahead of their end
    return templates, mf


def _run_staged(ra, ctx, band, templates, mf):
    tm = ra.Templates(ctx, [t for t in templates])
    ctx.dtw_kernels()
    before = ctx.dtw_ref_pairs()
    scores, _, agg = ctx.dtw_scores(mf, tm, band_size=band)
    listed = ctx.dtw_ref_pairs() - before
    assert "dtw_mfma_kernel" in ctx.dtw_kernels()
    return scores, agg, np.int64(listed)


def _run_live(ra, ctx, templates):
    from oracle import rp_oracle as orc
    _, L, T, cpc, chunks = LIVE
    tm = ra.Templates(ctx, [t for t in templates])
    cfg = ra.DetectorConfig()
    cfg.threshold, cfg.min_scores = 0.3, 1
    pcm = np.stack([orc.synth_pcm(SEED, 700 + s, 480 * chunks) for s in range(S)])
    sb = ra.StreamBatch(ctx, tm, cfg, S, max_chunks_per_call=cpc)
    ctx.dtw_kernels()
    rows = [sb.process(pcm[:, i:i + 480 * cpc], want_agg=True)[2] for i in range(0, pcm.shape[1], 480 * cpc)]
    assert "dtw_mfma_kernel" in ctx.dtw_kernels()
    return np.concatenate([np.asarray(r, np.float32).reshape(S, -1) for r in rows], axis=1)


def record(path):
    """Write the fixture with whatever library RP_LIB_PATH names: run with the library of the commit BEFORE the change."""
    from oracle import rp_oracle as orc
    import rustpotter_amd as ra
    out = {}
    for name in STAGED:
        out[name + "/templates"], out[name + "/mfcc"] = _inputs(name)
    out[LIVE[0] + "/templates"] = np.stack(orc.synth_templates(SEED + 99, LIVE[2], LIVE[1], 5))
    for arith in ARITHMETICS:
        ctx = ra.BatchContext(device=0, host_pointers=True, arithmetic=arith)
        for name, (band, L, T, special) in STAGED.items():
            scores, agg, listed = _run_staged(ra, ctx, band, out[name + "/templates"], out[name + "/mfcc"])
            assert np.isfinite(scores).all() and (listed > 0) == special, (name, listed)
            out["%s/%s/scores" % (arith, name)], out["%s/%s/agg" % (arith, name)], out["%s/%s/listed" % (arith, name)] = scores, agg, listed
        out["%s/%s/agg" % (arith, LIVE[0])] = _run_live(ra, ctx, out[LIVE[0] + "/templates"])
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module", params=ARITHMETICS)
def ctx(ra, request):
    return ra.BatchContext(device=0, host_pointers=True, arithmetic=request.param)


@pytest.mark.parametrize("name", list(STAGED))
def test_staged_tiles_give_the_recorded_bits(ra, ctx, golden, name):
    """Scores, the aggregate (ScoreMode::Max inside the kernel) and the number of pairs listed for dtw_ref_kernel (whose rescored rows are part
    of the scores: a window listed or left out by mistake changes bits) equal the fixture."""
    arith = ctx.get_arithmetic()[0]
    band, L, T, special = STAGED[name]
    scores, agg, listed = _run_staged(ra, ctx, band, golden[name + "/templates"], golden[name + "/mfcc"])
    assert scores.shape == (S, N_WIN, T)
    assert int(listed) == int(golden["%s/%s/listed" % (arith, name)]), (int(listed), int(golden["%s/%s/listed" % (arith, name)]))
    assert _same_bits(scores, golden["%s/%s/scores" % (arith, name)]), int((scores != golden["%s/%s/scores" % (arith, name)]).sum())
    assert _same_bits(agg, golden["%s/%s/agg" % (arith, name)])
    if special:
        assert int(listed) > 0


def test_live_stream_batch_gives_the_recorded_bits(ra, ctx, golden):
    """Three live streams fed two chunks per call: six new windows per stream, frames read from global memory."""
    arith = ctx.get_arithmetic()[0]
    agg = _run_live(ra, ctx, golden[LIVE[0] + "/templates"])
    want = golden["%s/%s/agg" % (arith, LIVE[0])]
    assert _same_bits(agg, want)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:2] == ["--record"]:
        record(sys.argv[2] if len(sys.argv) > 2 else GOLDEN)
