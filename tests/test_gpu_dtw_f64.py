"""Is the matrix-core DTW an f32-GRADE evaluation of the reference's scoring?  Three-way test: the scores of the kernel (through the C ABI),
of the strict-f32 oracle, and of an f64 evaluation of the same formula -- window cut + mean normalisation (wakeword_comp.rs:22-27,
normalizer.rs:3-31), cosine distance (comparator.rs:15-48), banded DTW read at D[m-1][n] (dtw.rs:56-105), cost / (m + n) -> logistic
(comparator.rs:18-26) -- on BASELINE C3's inputs (synthetic 16 kHz streams, 8 templates of 100 frames, mfcc_size 5, band 5, score_ref 0.22).

The oracle's own distance from the f64 value is what f32 arithmetic costs (the running sums of ~200 cell costs round at every add).  The bar
the default arithmetic (RP_ARITH_F32_MATRIX: operands as three bf16 parts, six partial products, f32 accumulate) has to meet is the one
round 5 set for the MFCC and the model forward: an rms error of at most 1.25 x the oracle's and a largest error of at most 1.25 x the
oracle's largest, over every score of the sample.  The strict-f32 vector kernels and the two-part f16 form (RP_ARITH_FAST_SPLIT, 22-bit
operands) run through the same measurement; their ratios are printed and bounded too, so the record says what each arithmetic is."""
import numpy as np
import pytest

from abandon_ref import f64_scores   # the f64 restatement (tests/abandon_ref.py; pinned on the CPU in tests/test_abandon_ref.py)
from oracle import rp_oracle as orc

SEED = 0x5EED000000000001
K, T, L, BAND, SCORE_REF = 5, 8, 100, 5, 0.22


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def sample(ra):
    """16 streams of BASELINE C3 (4 s each): kernel MFCC frames (what the DTW stage is handed), the oracle's and the f64 scores of those frames."""
    ctx = ra.BatchContext(device=0, host_pointers=True)
    S, N = 16, 64000
    templates = orc.synth_templates(SEED, T, L, K)
    pcm = ctx.synth_pcm(SEED, 0, S, N)
    mf = ctx.mfcc(pcm, K)
    ref = np.stack([orc.score_stream(mf[s], templates, BAND, SCORE_REF)[0] for s in range(S)]).astype(np.float64)
    tru = np.stack([f64_scores(mf[s], templates) for s in range(S)])
    tm = ra.Templates(ctx, templates)
    return ctx, mf, tm, ref, tru


def _errors(got, tru):
    e = np.abs(got - tru) / tru     # the parity contract is relative (1e-5 of a score)
    return float(np.sqrt((e * e).mean())), float(e.max()), float(((got - tru) / tru).mean())


def _measure(sample, arithmetic, expect_kernel, expect_products, min_size=16 * 297 * 8):
    ctx, mf, tm, ref, tru = sample
    with ctx.arithmetic(arithmetic):
        ctx.dtw_kernels()
        got = ctx.dtw_scores(mf, tm, score_ref=SCORE_REF, band_size=BAND)[0].astype(np.float64)
        ran = ctx.dtw_kernels()
    assert expect_kernel in ran, ran
    assert ctx.last_dtw_products == expect_products, ctx.last_dtw_products
    assert got.shape == ref.shape == tru.shape and got.size >= min_size
    k_rms, k_max, k_mean = _errors(got, tru)
    o_rms, o_max, o_mean = _errors(ref, tru)
    print("\n%-11s rel. score error vs f64: kernel rms %.3e max %.3e mean %+.2e | oracle rms %.3e max %.3e mean %+.2e | ratio rms %.3f max %.3f | kernel vs oracle max %.3e"
          % (arithmetic, k_rms, k_max, k_mean, o_rms, o_max, o_mean, k_rms / o_rms, k_max / o_max, float((np.abs(got - ref) / ref).max())))
    assert np.all(np.abs(got - ref) <= 1e-5 * ref), "the 1e-5 parity contract against the oracle"
    return k_rms / o_rms, k_max / o_max


@pytest.mark.gpu
def test_f32_matrix_scores_are_f32_grade(sample):
    """The default arithmetic: three bf16 parts per operand on the matrix cores.  As good an f32 evaluation as the oracle itself."""
    r_rms, r_max = _measure(sample, "f32_matrix", "dtw_mfma_kernel", ["bf16x3"])
    assert r_rms <= 1.25 and r_max <= 1.25, (r_rms, r_max)


@pytest.mark.gpu
@pytest.mark.parametrize("K_, T_, kernel", [(5, 4, "dtw_mfma_kernel"), (5, 3, "dtw_mfma_kernel"), (16, 8, "dtw_mfma_wide_kernel"), (13, 5, "dtw_mfma_wide_kernel")])
def test_the_other_three_part_shapes_are_f32_grade(ra, K_, T_, kernel):
    """The same bar for the other kernels of the default arithmetic: the four-slot shape of dtw_mfma_kernel (chunks of 3..4 templates) and
    dtw_mfma_wide3_kernel (mfcc_size 13 / 16: six k-steps of three-part products, reported as dtw_mfma_wide_kernel + bf16x3)."""
    ctx = ra.BatchContext(device=0, host_pointers=True)
    S, N = 16, 64000
    templates = orc.synth_templates(SEED + 31 * K_ + T_, T_, L, K_)
    pcm = ctx.synth_pcm(SEED, 100, S, N)
    mf = ctx.mfcc(pcm, K_)
    ref = np.stack([orc.score_stream(mf[s], templates, BAND, SCORE_REF)[0] for s in range(S)]).astype(np.float64)
    tru = np.stack([f64_scores(mf[s], templates) for s in range(S)])
    # through the batched detector (the wide kernels read their frames from rows with slack behind them: the library's own MFCC buffer)
    cfg = ra.DetectorConfig()
    cfg.avg_threshold, cfg.score_ref, cfg.band_size = 0.0, SCORE_REF, BAND
    tm = ra.Templates(ctx, templates)
    ctx.dtw_kernels()
    got = ctx.batch_detect(pcm, tm, cfg, want_scores=True)[2].astype(np.float64)
    assert kernel in ctx.dtw_kernels() and ctx.last_dtw_products == ["bf16x3"]
    assert got.shape == ref.shape == tru.shape == (S, 297, T_)
    assert np.all(np.abs(got - ref) <= 1e-5 * ref), "the 1e-5 parity contract against the oracle"
    k_rms, k_max, _ = _errors(got, tru)
    o_rms, o_max, _ = _errors(ref, tru)
    print("\nmfcc_size %d, %d templates: rel. score error vs f64: kernel rms %.3e max %.3e | oracle rms %.3e max %.3e | ratio rms %.3f max %.3f"
          % (K_, T_, k_rms, k_max, o_rms, o_max, k_rms / o_rms, k_max / o_max))
    assert k_rms <= 1.25 * o_rms and k_max <= 1.25 * o_max, (k_rms / o_rms, k_max / o_max)


@pytest.mark.gpu
def test_strict_f32_vector_kernels(sample):
    """The f32 vector kernels (unit vectors + an FMA chain from 1 per cell): the same measurement, for the record."""
    r_rms, r_max = _measure(sample, "strict_f32", "register kernels", [])
    assert r_rms <= 1.6 and r_max <= 2.0, (r_rms, r_max)


@pytest.mark.gpu
def test_fast_split_is_recorded_as_narrower(sample):
    """Two f16 parts per operand (22 bits, x1 a1 dropped): inside the parity contract, not claimed to be f32-grade -- the ratio is printed
    and only bounded loosely."""
    r_rms, r_max = _measure(sample, "fast_split", "dtw_mfma_kernel", ["f16x2"])
    assert r_rms <= 3.0 and r_max <= 4.0, (r_rms, r_max)


def test_f64_evaluation_agrees_with_the_oracle_on_a_golden_shape():
    """The f64 restatement itself, pinned on CPU-checkable ground: against the strict-f32 oracle within f32 rounding on random frames with
    templates of unequal lengths and another band (catches an off-by-one in the band or the read-out cell)."""
    rng = np.random.default_rng(7)
    mf = rng.standard_normal((180, K)).astype(np.float32) * 3 + 1
    templates = [(rng.standard_normal((n, K)) * 2).astype(np.float32) for n in (40, 57, 33)]
    for band in (3, 5, 7):
        tru = []
        for tpl in templates:
            s = f64_scores(mf, [tpl], band=band)[:, 0]
            tru.append(s)
        ref = orc.score_stream(mf, templates, band, SCORE_REF)[0]
        n_win = ref.shape[0]   # the oracle scores the windows every template fits in
        for t in range(3):
            assert np.allclose(tru[t][:n_win], ref[:, t], rtol=3e-6, atol=0), (band, t)
