"""Every build of the register DTW kernels (rp_dtw.hip over csrc/rp_dtw_lane.h), at the lengths and tile edges where the per-lane walk can go
wrong, in each of its four lane -> window forms.

The context runs arithmetic="strict_f32", so the register kernels score every template set (no matrix-core kernel takes a chunk).  Which
instantiation a set takes follows from its chunk classes (Templates::create; launch_dtw_k5 / launch_dtw_wide_all, rp_dtw.hip):

  mfcc_size 5    t1      one template                 dtw_band2_kernel<5, W>       (two windows per lane, waves of 128 entries)
                 t2      two of one length            dtw_band_kernel<5, W, 2>
                 t4      four of one length           dtw_band_kernel<5, W, 4>
                 t8      eight of one length          dtw_band_kernel<5, W, 8>     (RP_DTW_NO_SPLIT=1: a batch this small would take <5, W, 4> halves)
                 ragged  lengths 2W, 2W + 2, 40       dtw_band2_kernel<5, W>, three chunks of different lengths in one launch
  mfcc_size 13 / 16
                 t1      one template                 dtw_band_wide_kernel<K, W, 1>
                 t2      two of one length            dtw_band_wide_kernel<K, W, 2>
                 t3      three of one length          dtw_band_wide_kernel<K, W, 2> and <K, W, 1> (a pair plus a single)

Lengths: L = 2W (only the guarded block of rows, cut by r < L), 2W + 1 and 2W + 2 (the first abandon check, a second block of one row), 40.
Windows per stream on the tile edges: 1, 63, 64, 65, 130, and 127, 128, 129 for the two-windows-per-lane kernel.

The four forms and how they are reached:
  staged, per-stream tiles   rp_dtw_score_batch (rows without slack: never the global-memory form), one stream, or streams shorter than a tile
  staged, flat tiling        the same with three streams of at least one full tile: waves straddle two streams (the wide kernels have no flat
                             tiling: their three-stream calls are per-stream tiles too)
  global memory              rp_batch_detect with per-window scores over streams of fewer than 64 windows
  list mode                  a detect-only rp_batch_detect behind the averaged-template gate with every row listed, read back from the workspace
(One stream of at most 8 windows belongs to dtw_single_kernel: the one-window calls here have three streams.)

Checks: (a) every score within the parity contract of the C oracle, |got - ref| <= 1e-5 * ref; (b) the forms give bit-equal scores for the same
windows; (c) the sha256 of the score bits of the staged calls equals tests/golden/register_dtw_bits.json.  For (c) the frames are built here
from integer arithmetic (exact in f32; no library RNG, no GPU stage in front), so the fixture depends on the DTW alone.  With -ffp-contract=off
and explicit FMAs a refactor of the kernels performs the same operations in the same order: a changed hash is a bug, not rounding.  A change
that moves the arithmetic on purpose re-records the fixture (RP_REGISTER_DTW_RECORD=<file> writes the hashes of this run there instead of
comparing them) and says so.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import rp_oracle as orc

SCORE_REF = 0.22
REG = "register kernels"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "register_dtw_bits.json")
N_WIN = (1, 63, 64, 65, 130)
N_WIN_2 = (1, 63, 64, 65, 127, 128, 129, 130)      # dtw_band2_kernel: tiles of 128 entries
KW = [(K, W) for K in (5, 13, 16) for W in (3, 4, 5, 6)]
RECORDED = {}


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True, arithmetic="strict_f32")


@pytest.fixture(autouse=True)
def no_split(monkeypatch):
    monkeypatch.setenv("RP_DTW_NO_SPLIT", "1")      # read per call: eight templates stay dtw_band_kernel<5, W, 8>


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def int_frames(stream, nf, K):
    """frames of integer arithmetic: residues of a quadratic in (frame, component, stream) modulo a prime, centred, in 32nds -- exact in f32"""
    f = np.arange(nf, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    s = int(stream)
    x = (37 * f * f + 101 * f * (k + 1) + 53 * k * k + 11 * f * (s + 3) + 7919 * (s + 1) + 29 * (k + 2) * (s + 5)) % 251
    return ((x - 125) / 32.0).astype(np.float32)


def sets_of(K, W):
    """(name, template lengths, windows per stream to run) of one (mfcc_size, band); see the table at the head of the file"""
    out = []
    for L in (2 * W, 2 * W + 1, 2 * W + 2, 40):
        if K == 5:
            out += [("t1_L%d" % L, [L], N_WIN_2), ("t2_L%d" % L, [L] * 2, N_WIN), ("t4_L%d" % L, [L] * 4, N_WIN), ("t8_L%d" % L, [L] * 8, N_WIN)]
        else:
            out += [("t1_L%d" % L, [L], N_WIN), ("t2_L%d" % L, [L] * 2, N_WIN), ("t3_L%d" % L, [L] * 3, N_WIN)]
    if K == 5:
        out.append(("ragged", [2 * W, 2 * W + 2, 40], N_WIN_2))
    return out


def assert_inside_norm_range(mf, L, W):
    """the premise of a case: every frame a window's walk loads -- its own L and the W - 2 behind its end, zeros past the stream -- keeps a
    centred squared norm far inside kDtwNormLo..kDtwFixLimit (2^-60 .. 2^30), so nothing is listed for dtw_ref_kernel"""
    S, nf, K = mf.shape
    x = np.concatenate([mf.astype(np.float64), np.zeros((S, W, K))], axis=1)
    for w in range(nf - L + 1):
        y = x[:, w:w + L + W - 1] - x[:, w:w + L].mean(axis=1, keepdims=True)
        bb = (y * y).sum(axis=2)
        assert bb.min() > 1e-3 and bb.max() < 1e4, (w, bb.min(), bb.max())


def scored(ra, ctx, fn):
    """run one scoring call: the register kernels ran and no pair was re-scored by dtw_ref_kernel (it would overwrite what is under test)"""
    pairs = ctx.dtw_ref_pairs()
    ctx.dtw_kernels()
    got = fn()
    ran = ctx.dtw_kernels()
    assert REG in ran, ran
    assert ctx.dtw_ref_pairs() == pairs
    return got


def assert_parity(got, ref, where):
    assert got.shape == ref.shape, (where, got.shape, ref.shape)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 1e-5 * ref), (where, float((np.abs(got - ref) / ref).max()))


# ------------------------------------------------------------------ the staged forms on integer frames: (a), (b), (c)
@pytest.mark.gpu
@pytest.mark.parametrize("K,W", KW, ids=["K%d_band%d" % kw for kw in KW])
def test_staged_forms_on_integer_frames(ra, ctx, K, W):
    for name, lens, n_wins in sets_of(K, W):
        Lmax = max(lens)
        templates = [int_frames(100 + t, n, K) for t, n in enumerate(lens)]
        assert min(float((t.astype(np.float64) ** 2).sum(axis=1).min()) for t in templates) > 1e-2     # rows inside the norm range
        tm = ra.Templates(ctx, templates)
        nf_max = max(n_wins) + Lmax - 1
        mf3 = np.stack([int_frames(s, nf_max, K) for s in range(3)])
        for n in sorted(set(lens)):
            assert_inside_norm_range(mf3, n, W)
        ref = np.stack([orc.score_stream(mf3[s], templates, W, SCORE_REF)[0] for s in range(3)]).astype(np.float64)
        h = hashlib.sha256()
        base = None
        for n_win in sorted(n_wins, reverse=True):
            nf = n_win + Lmax - 1
            for S in ((3, 1) if n_win > 8 else (3,)):       # one stream of <= 8 windows is dtw_single_kernel's
                where = (K, W, name, n_win, S)
                got = scored(ra, ctx, lambda: ctx.dtw_scores(mf3[:S, :nf], tm, score_ref=SCORE_REF, band_size=W)[0])
                assert_parity(got, ref[:S, :n_win], where)                                         # (a)
                if base is None:
                    base = got
                # (b) per-stream tiles (S = 1, or a tile's worth of windows not reached) and the flat tiling (S = 3): a window's bits depend
                # on neither the tiling nor the lane it falls on
                assert np.array_equal(_bits(got), _bits(base[:S, :n_win])), (where, np.argwhere(_bits(got) != _bits(base[:S, :n_win]))[:4])
                h.update(_bits(got).tobytes())
        RECORDED["K%d_band%d_%s" % (K, W, name)] = h.hexdigest()
    if not os.environ.get("RP_REGISTER_DTW_RECORD"):                                               # (c)
        golden = json.load(open(GOLDEN))
        mine = {k: v for k, v in RECORDED.items() if k.startswith("K%d_band%d_" % (K, W))}
        assert mine and all(golden.get(k) == v for k, v in mine.items()), sorted(k for k, v in mine.items() if golden.get(k) != v)


# ------------------------------------------------------------------ the global-memory and list-mode forms against the staged one: (a), (b)
@pytest.mark.gpu
@pytest.mark.parametrize("K,W", KW, ids=["K%d_band%d" % kw for kw in KW])
def test_global_and_list_forms_match_the_staged_form(ra, ctx, K, W):
    """11 streams of 12 to 14 windows: 3 partial-ended tiles of 64 entries, 2 of 128.  The same MFCC frames (the library's own, from synthetic PCM:
    rp_batch_detect has no frame input) are scored staged (rp_dtw_score_batch), from global memory (rp_batch_detect with scores) and in list
    mode (detect-only behind the averaged-template gate at a threshold every row passes; threshold 0: no early abandon)."""
    S = 11
    for L in (2 * W + 2, 40):
        chunks = (L + 11 + 3 + 2) // 3
        pcm = ctx.synth_pcm(0x5EED000000000001, 500 + L, S, 480 * chunks)
        mf = ctx.mfcc(pcm, K)
        nf = mf.shape[1]
        n_win = nf - L + 1
        assert 12 <= n_win <= 14 and (S * n_win) % 64 != 0
        for T in ((1, 2, 4, 8) if K == 5 else (1, 2, 3)):
            where = (K, W, L, T)
            templates = list(orc.synth_templates(0x5EED000000000001 + 31 * K + 7 * L + W, T, L, K))
            ref = np.stack([orc.score_stream(mf[s], templates, W, SCORE_REF)[0] for s in range(S)]).astype(np.float64)
            tm = ra.Templates(ctx, templates)
            staged = scored(ra, ctx, lambda: ctx.dtw_scores(mf, tm, score_ref=SCORE_REF, band_size=W)[0])
            assert_parity(staged, ref, where)
            cfg = ra.DetectorConfig()
            cfg.avg_threshold, cfg.threshold, cfg.min_scores, cfg.band_size, cfg.score_ref = 0.0, 0.0, 1, W, SCORE_REF
            glob = scored(ra, ctx, lambda: ctx.batch_detect(pcm, tm, cfg, max_det=1, want_scores=True)[2])
            assert np.array_equal(_bits(glob), _bits(staged)), (where, "global memory", np.argwhere(_bits(glob) != _bits(staged))[:4])
            tg = ra.Templates(ctx, templates, avg=np.mean(templates, axis=0, dtype=np.float32))
            cfg.avg_threshold = 1e-30       # a score is > 0: every row is listed; few windows per stream: list mode only (dense_min = 0)

            def listed():
                ctx.batch_detect(pcm, tg, cfg, max_det=1)
                return ctx.last_window_scores(S, n_win, T)
            lst = scored(ra, ctx, listed)
            assert np.array_equal(_bits(lst), _bits(staged)), (where, "list mode", np.argwhere(_bits(lst) != _bits(staged))[:4])


# ------------------------------------------------------------------ the record
@pytest.mark.gpu
def test_write_the_recorded_hashes():
    """Runs last: with RP_REGISTER_DTW_RECORD=<file> the hashes of this run are written there (tests/golden/register_dtw_bits.json)."""
    path = os.environ.get("RP_REGISTER_DTW_RECORD")
    if not path or not RECORDED:
        return
    with open(path, "w") as f:
        json.dump(dict(sorted(RECORDED.items())), f, indent=0)
        f.write("\n")
