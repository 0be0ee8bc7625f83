"""The score_mode aggregate behind rp_dtw_score_batch at every code path of launch_aggregate (rp_dtw.hip): aggregate_kernel (Max and
Average, the tile in LDS), the six aggregate_sorted_reg_kernel<NT> builds (bitonic sort in registers, NT = 2 .. 64) and
aggregate_sorted_kernel (insertion sort in scratch memory, 65 .. 256 templates) -- at both sides of every dispatch boundary, at the
largest template count, and at the counts where the percentile position p/100 * (T-1), formed in f32, is a whole number for some or
all modes (T - 1 = 5, 10, 15: P80; 20, 100: all six), which decides between "take the element" and "interpolate".

The witness is the CPU oracle's aggregate of the GPU's OWN per-template scores of the same call, bit for bit: DTW precision does not
enter, no tolerance is involved.  Scores are finite here; where NaN scores sort is outside this test -- the kernels' min/max network
and `>` insertion order differ from the reference's total_cmp for NaN by design (comment at aggregate_sorted_kernel)."""
import numpy as np
import pytest

from oracle import rp_oracle as orc

pytestmark = pytest.mark.gpu

SEED = 0x5EED000000000001
K, N_WIN, MAX_LEN, T_MAX = 5, 43, 16, 256
COUNTS = [1, 2, 3, 4, 5, 6, 8, 9, 11, 16, 17, 21, 32, 33, 41, 64, 65, 81, 101, 255, 256]
MODES = ["average", "max", "median", "p25", "p50", "p75", "p80", "p90", "p95"]


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


@pytest.fixture(scope="module")
def templates():
    """T_MAX + 1 templates of 12 .. 16 frames, the first one 16 long (every prefix of the list has 16-frame windows); every fourth one,
    from the fourth on, is an exact copy of the template three places before it: rows of four or more scores hold equal values"""
    base = orc.synth_templates(SEED + 77, T_MAX + 1, MAX_LEN, K)
    out = []
    for i, t in enumerate(base):
        out.append(out[i - 3].copy() if i % 4 == 3 else t[: MAX_LEN if i == 0 else 12 + (i * 7) % 5].copy())
    return out


@pytest.fixture(scope="module")
def frames():
    """3 streams x 58 frames = 3 x 43 windows = 129 rows: two full blocks of 64 rows and one row in a third.  Stream 1 is digitally
    silent for 13 chunks: its windows there normalise to exactly 0, every DTW cell costs 1 and all templates score the same"""
    n = 480 * 21
    pcm = np.stack([orc.synth_pcm(SEED, 40 + s, n) for s in range(3)])
    pcm[1, 480 * 4:480 * 17] = 0.0
    mf = np.stack([orc.mfcc_stream(pcm[s], K) for s in range(3)])[:, :N_WIN + MAX_LEN - 1]
    assert mf.shape == (3, 58, K)
    return np.ascontiguousarray(mf)


@pytest.mark.parametrize("T", COUNTS)
def test_every_aggregate_build_bit_for_bit(ra, ctx, templates, frames, T):
    tm = ra.Templates(ctx, templates[:T])
    assert tm.max_len == MAX_LEN
    seen_equal = seen_duplicates = False
    for mode in MODES:
        sm = {m.name.lower(): m for m in ra.ScoreMode}[mode]
        scores, _, agg = ctx.dtw_scores(frames, tm, score_mode=sm)
        assert scores.shape == (3, N_WIN, T) and agg.shape == (3, N_WIN) and np.isfinite(scores).all()
        rows = scores.reshape(-1, T)
        assert rows.shape[0] == 129
        ref = np.array([orc.aggregate(r, mode) for r in rows], np.float32)
        got = agg.reshape(-1)
        bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
        assert bad.size == 0, (T, mode, "rows", bad[:8], got[bad[:4]], ref[bad[:4]])
        distinct = np.array([len(np.unique(r)) for r in rows])
        seen_equal = seen_equal or bool((distinct == 1).any())
        seen_duplicates = seen_duplicates or bool(((distinct > 1) & (distinct < T)).any())
    # the input really holds what it was built for (T = 1: a row of one score is trivially all-equal)
    assert seen_equal, "no row of equal scores: the silent stretch did not reach the windows"
    if T >= 4:
        assert seen_duplicates, "no row with some equal scores: the copied templates did not score alike"


def test_more_templates_than_the_aggregate_takes(ra, ctx, templates, frames):
    """257 templates: the set can be created (its per-template scores can be had without an aggregate), the scoring call that asks for
    the aggregate is refused before anything runs, with the limit in the message"""
    tm = ra.Templates(ctx, templates[:T_MAX + 1])
    with pytest.raises(ra.RustpotterError, match="257 templates exceeds the 256-template limit"):
        ctx.dtw_scores(frames, tm)
    cfg = ra.DetectorConfig()
    with pytest.raises(ra.RustpotterError, match="257 templates exceeds the 256-template limit"):
        ctx.batch_detect(np.zeros((2, 480 * 21), np.float32), tm, cfg)
    # the context is usable afterwards
    tm = ra.Templates(ctx, templates[:T_MAX])
    _, _, agg = ctx.dtw_scores(frames, tm)
    assert agg.shape == (3, N_WIN) and np.isfinite(agg).all()
