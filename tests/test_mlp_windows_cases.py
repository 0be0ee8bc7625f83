"""The case table of tests/test_gpu_mlp_windows_builds.py proves its own coverage here, without a GPU: through the restated cut and route it
reaches each of the 30 builds of the staged-frame window kernels and the named route edges; the f32 oracle stays within a quarter of the
project's logit gate from the f64 reference on every case, so the gate is not busy absorbing the reference's own rounding; and on the
partial-product cases the emulation of the kernels' product sets passes the gate of those cases, while leaving one product out misses it by
the margins mlp_windows_cases.py derives."""
import numpy as np
import pytest

import mlp_windows_cases as M


def test_cut_restates_the_known_shapes():
    """the figures DESIGN.md 4.4 and rp_mlp.hip quote: 205 windows are one workgroup of seven tiles, 300 two of five; the multi-workgroup
    cuts the table relies on; the wide form's two or four tiles"""
    assert M.cut(205) == (7, 1) and M.cut(300) == (5, 2) and M.cut(0) == (0, 0) and M.cut(1) == (1, 1)
    assert [M.cut(n) for n in (224, 225, 257, 353, 417, 449, 673)] == [(7, 1), (4, 2), (5, 2), (6, 2), (7, 2), (5, 3), (6, 4)]
    assert M.workgroups(257, 5) == [(0, 160), (160, 97)] and M.workgroups(673, 6)[-1] == (576, 97)
    assert M.cut(225, 3) == (3, 3) and M.workgroups(225, 3) == [(0, 96), (96, 96), (192, 33)] and M.cut(225, 6) == (4, 2)
    assert [M.wide_cut(n) for n in (32, 33, 64, 65, 128, 129, 161, 192, 257)] == [(2, 1), (2, 1), (2, 1), (4, 1), (4, 1), (4, 2), (4, 2), (4, 2), (4, 3)]
    for n_win in range(1, 1500):        # every window belongs to exactly one workgroup, none owns more than its build's tiles, none is empty
        for nt, bps in (M.cut(n_win), M.wide_cut(n_win), M.cut(n_win, 3)):
            wgs = M.workgroups(n_win, nt)
            assert len(wgs) == bps and sum(r for _, r in wgs) == n_win and all(0 < r <= nt * 32 for _, r in wgs) and 1 <= nt <= 7


def test_route_restates_the_known_routes():
    """the routes tests/test_gpu_mlp_range_and_windows.py already pins on the device (test_mlp_route_table_windows), and the 160-output single
    layer that Model::create leaves to the per-layer kernel"""
    inp = 16 * 195
    assert M.route((inp, 32, 16, 2), 16, 40, "f32")[:3] == ("mlp_windows_kernel<bf16x3 splits>", 2, 0)
    assert M.route((inp, 32, 16, 2), 16, 40, "bf16")[0] == "mlp_windows_kernel<bf16x3 splits>"
    assert M.route((inp, 65, 32, 2), 16, 40, "f32_fast")[:3] == ("mlp_windows_wide_kernel<f16x2 splits>" + M.LISTED, 2, 3)
    assert M.route((inp, 32, 16, 2), 16, 31, "f32_fast")[0] == "mlp_mfma_kernel<f16x2 splits>, windows read in place," + M.LISTED
    assert M.route((inp, 32, 16, 2), 16, 40, "f32_strict")[0] == "mlp_mfma_kernel<f32 matrix instructions>, windows read in place"
    assert M.route((inp, 32, 16, 2), 16, 40, "f32", windows_env="0")[0] == "mlp_mfma_kernel<bf16x3 splits>, windows read in place"
    assert M.route((inp, 144, 64, 2), 16, 40, "f32")[0] == "mlp_mfma_kernel<f32 matrix instructions>, windows read in place"
    assert M.route((inp, 144, 64, 2), 16, 40, "f32_fast")[0] == "mlp_mfma_kernel<f16x2 splits>, windows read in place," + M.LISTED
    assert M.route((480, 160), 16, 41, "f32") == (None, 0, 0, 0, 0)
    assert M.route((480, 144), 16, 41, "f32") == ("mlp_windows_wide_kernel<bf16x3 splits>", 2, 5, 1, 41)
    assert M.route((16 * 20, 130, 32, 3), 16, 236, "f32")[1:] == (4, 5, 2, 108)
    assert M.route((32, 32, 16, 2), 16, 65, "f32")[:2] == ("mlp_windows_kernel<bf16x3 splits>", 3)
    assert M.route((16, 32, 16, 2), 16, 65, "f32") == ("mlp_mfma_kernel<bf16x3 splits>, windows read in place", 0, 0, 0, 0)      # one frame


def test_table_reaches_every_build_and_edge():
    builds = {}
    for case in M.CASES:
        name, nt, nq, bps, last = M.route_of(case)
        if case[0] == 1:        # windows of one frame: mlp_mfma_kernel, the row's own mean
            assert name.startswith("mlp_mfma_kernel<") and "windows read in place" in name and nt == 0, case
            continue
        assert name.startswith("mlp_windows_wide_kernel<" if nq else "mlp_windows_kernel<") and nt > 0, case
        builds.setdefault(M.build_of(case), []).append(case)
    assert set(builds) == M.ALL_BUILDS and len(M.ALL_BUILDS) == 30
    by = lambda **kw: [c for c in M.CASES if all({"L": c[0], "hidden": c[1], "labels": c[2], "n_win": c[3], "prec": c[4]}[k] == v for k, v in kw.items())]
    shape = lambda c: M.route_of(c)[1:]
    for prec in M.PRECISIONS:
        # narrow: NT 1..7 with a last tile of one row and of 32 rows
        got = {(shape(c)[0], c[3] % 32) for c in M.CASES if shape(c)[1] == 0 and shape(c)[2] == 1 and c[4] == prec}
        assert got >= {(nt, r) for nt in range(2, 8) for r in (0, 1)} | {(1, 0)}
        # several workgroups: a wholly empty trailing tile (97 rows of NT 5 and of NT 6), three and four workgroups
        multi = {shape(c) for c in M.MULTI if c[4] == prec}
        assert multi >= {(4, 0, 2, 97), (5, 0, 2, 97), (6, 0, 2, 161), (7, 0, 2, 193), (5, 0, 3, 129), (6, 0, 4, 97)}
        # wide: every NQ at NT 2 (partial and full), NT 4 with an empty fourth tile, full, and last workgroups of one row
        for nq in (2, 3, 4, 5):
            assert multi >= {(4, nq, 2, 1), (4, nq, 3, 1), (4, nq, 2, 33), (4, nq, 2, 64)}
            assert {shape(c) for c in M.CASES if c[4] == prec} >= {(2, nq, 1, 33), (2, nq, 1, 64), (4, nq, 1, 65), (4, nq, 1, 128)}
        # window lengths, the longest in both forms
        assert {c[0] for c in by(prec=prec, hidden=(32, 16), n_win=65)} >= {1, 2, 3, 4, 5, 13}
        assert by(L=256, prec=prec, n_win=224, hidden=(32, 16)) and by(L=256, prec=prec, n_win=128, hidden=(65, 32))
    assert {c[0] for c in by(hidden=(65, 32), n_win=65)} >= {1, 2, 3, 4, 5, 13}
    # layer-1 widths on both sides of every tile edge, model depths, tail widths and label counts
    assert {M.dims_of(c)[1] for c in M.CASES} >= {1, 16, 17, 32, 33, 64, 65, 96, 97, 128, 129, 144}
    assert {len(M.dims_of(c)) - 1 for c in M.CASES if shape(c)[1] == 0} == {1, 2, 3} == {len(M.dims_of(c)) - 1 for c in M.CASES if shape(c)[1]}
    assert {d for c in M.CASES for d in M.dims_of(c)[2:-1]} >= {1, 3, 31, 32} and {c[2] for c in M.CASES} >= {1, 2, 32}
    assert all(M.streams_of(c) == (1 if c[0] == 256 else 2) for c in M.CASES)
    assert max(M.streams_of(c) * (c[3] + c[0] - 1) for c in M.CASES) <= 2 * 680       # the streams stay small
    # the route edges: mlp_mfma_kernel reading the windows in place, or (layer 1 beyond 144) the per-layer kernel
    for edge in M.EDGES:
        name = M.route_of(edge)[0]
        wide = M.dims_of(edge, edge[5])[1]
        assert (name is None) == (wide > 144) and (name is None or (name.startswith("mlp_mfma_kernel<") and "windows read in place" in name)), edge
    assert {(e[0] > 256, M.dims_of(e, e[5])[1] > 144, max(e[1][1:] + (0,)) > 32, e[3] < 32, e[5] != 16) for e in M.EDGES} == \
        {(True, False, False, False, False), (False, True, False, False, False), (False, False, True, False, False),
         (False, False, False, True, False), (False, False, False, False, True)}
    assert {M.dims_of(e, e[5])[1] for e in M.EDGES} >= {145, 160}


@pytest.mark.parametrize("part", range(4))
def test_the_oracle_stays_within_a_quarter_of_the_gate(part):
    """|f32 oracle - f64 reference| <= gate / 4 on every case of the table (and the edges): what is left of the gate belongs to the kernels"""
    for case in (M.CASES + M.EDGES)[part::4]:
        mfcc, ws, bs = M.inputs_of(case)
        ref = M.reference_of(case)
        assert ref.shape == (M.streams_of(case), case[3], case[2]) and np.isfinite(ref).all()
        worst = float((np.abs(M.oracle(mfcc, case[0], ws, bs) - ref) / M.gate(ref, mfcc, case[0])).max())
        assert worst <= 0.25, (case, worst)


def test_the_emulation_agrees_with_the_reference():
    """emulate() with nothing left out is the forward: within the logit gate of the f64 reference on ordinary inputs of both forms and both
    arithmetics, several workgroups included (it restates the staging about the middle window's mean and the correction behind it)"""
    for case in [c for c in M.CASES if c[0] == 20 and c[3] in (97, 129, 257)][:8]:
        mfcc, ws, bs = M.inputs_of(case)
        ref = M.reference_of(case)
        worst = float((np.abs(M.emulate(mfcc, (ws, bs), case[4]) - ref) / M.gate(ref, mfcc, case[0])).max())
        assert worst <= (0.05 if case[4] == "f32" else 0.5), (case, worst)


def test_splits_restate_the_kernels():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(4096) * 10.0 ** rng.uniform(-3, 3, 4096)).astype(np.float32)
    for parts in (M.split_bf16x3(x), M.split_bf16x3_host(x)):
        assert all((M._bits(p) & 0xffff == 0).all() for p in parts)                                   # three bf16 values
        assert (sum(p.astype(np.float64) for p in parts) == x).all()                                  # exact
    t0, t1, t2 = M.split_bf16x3(x)
    assert (np.abs(t0) <= np.abs(x)).all() and (np.sign(t1) * np.sign(x) >= 0).all()                  # truncating: the parts share x's sign
    h0, h1, _ = M.split_bf16x3_host(x)
    assert (np.abs(x - h0) <= np.abs(x - t0)).all() and (h1 * x < 0).any()                            # rounded: nearer, and on either side
    one = np.array([np.float32(2.0) - np.float32(2.0 ** -23)])
    assert [float(p[0]) for p in M.split_bf16x3_host(one)] == [2.0, -2.0 ** -23, 0.0]                  # all mantissa bits set: nothing behind w1
    f0, f1 = M.split_f16x2_frames(x)
    w0, w1 = M.split_f16x2_weights(x)
    for a, b in ((f0, f1), (w0, w1)):
        assert (a.astype(np.float16).astype(np.float32) == a).all() and (b.astype(np.float16).astype(np.float32) == b).all()
    assert (np.abs(f0) <= np.abs(x)).all() and (np.abs(x - f0 - f1) <= np.abs(x) * 2.0 ** -21 + 2.0 ** -24).all()
    assert (np.abs(x - w0) <= np.abs(x - f0)).all() and (np.abs(x.astype(np.float64) - w0 - w1) <= np.abs(x) * 2.0 ** -22 + 2.0 ** -25).all()


@pytest.mark.parametrize("d1,n_win,prec,pattern", M.PARTS_CASES)
def test_a_missing_product_misses_the_gate(d1, n_win, prec, pattern):
    """The partial-product cases: the premises (all mantissa bits set, exponents in [0.5, 4), column sums exactly 0, one sign per product
    class), the full emulation within a quarter of the gate, and every product the pattern can show (PARTS_SHOW) missing it by at least 8x
    on EVERY window when left out.  The second-order products of the three-part form cannot: their figures, as derived in
    mlp_windows_cases.py -- x2 w0 1.8x, x1 w1 0.8x, x0 w2 0.45x on the "parts" pattern -- are asserted as they are."""
    mfcc, ws, bs = M.parts_inputs(d1, n_win, pattern)
    L = M.PARTS_L
    name, nt, nq, bps, _ = M.route((16 * L, d1), 16, n_win, prec)
    assert (nt, nq, bps) == ((3, 0, 1) if d1 == 32 else (4, 3, 1))
    assert (M._bits(mfcc) & 0x7fffff == 0x7fffff).all() and (np.abs(mfcc) >= 0.5).all() and (np.abs(mfcc) < 4).all()
    assert (M._bits(ws[0]) & 0x7fffff == M.PARTS_PATTERNS[pattern]).all() and (np.abs(ws[0]) >= 0.5).all() and (np.abs(ws[0]) < 4).all()
    for m in mfcc:
        assert (M.window_means(m, L) == 0).all()
        terms = np.lib.stride_tricks.sliding_window_view(m, L, axis=0).transpose(0, 2, 1).reshape(n_win, 1, -1) * ws[0][None, :4, :]
        assert ((terms > 0).all(axis=2) | (terms < 0).all(axis=2)).all()
    ref = M.reference(mfcc, L, ws, bs)
    mag = M.parts_magnitudes(mfcc, ws)
    assert (np.abs(ref) <= mag).all() and (np.abs(ref) >= 0.999 * mag).all()         # nothing cancels
    t = M.parts_truncation(mfcc, ws, prec)
    assert t <= (1.5 if prec == "f32" else 7.0) * 2.0 ** -24
    gate = M.parts_gate(mfcc, ws, prec)
    assert (np.abs(M.emulate(mfcc, (ws, bs), prec) - ref) <= 0.25 * gate).all()
    ratio = {p: np.abs(M.emulate(mfcc, (ws, bs), prec, drop=p) - ref) / gate for p in M.PRODUCTS[prec]}
    for p in M.PARTS_SHOW[prec, pattern]:
        assert ratio[p].min() >= 8.0, (p, float(ratio[p].min()))
    if prec == "f32":
        assert 1.8 <= ratio["x2w0"].min() <= ratio["x2w0"].max() <= 1.9
        if pattern == "parts":
            assert 0.8 <= ratio["x1w1"].min() <= ratio["x1w1"].max() <= 0.95 and 0.45 <= ratio["x0w2"].min() <= ratio["x0w2"].max() <= 0.5


def test_every_product_shows_on_some_pattern():
    """PARTS_SHOW between its patterns names every product of the two-part form and every product of the three-part form up to first order"""
    for prec, want in (("f32", {"x0w0", "x1w0", "x0w1"}), ("f32_fast", set(M.PRODUCTS["f32_fast"]))):
        assert set().union(*[M.PARTS_SHOW[prec, pat] for pat in M.PARTS_PATTERNS]) == want
    assert set(M.PRODUCTS["f32"]) - {"x0w0", "x1w0", "x0w1"} == {"x2w0", "x1w1", "x0w2"}


def test_hot_frame_cases_sit_inside_the_middle_window():
    for hidden, n_win, prec, value in M.HOT_CASES:
        name, nt, nq, bps, _ = M.route((16 * M.HOT_L,) + hidden + (2,), 16, n_win, prec)
        w0, rows = M.workgroups(n_win, nt)[0]
        hot = M.hot_frame(n_win, nt)
        mid = w0 + rows // 2
        assert mid <= hot < mid + M.HOT_L and hot + 1 <= rows              # in the middle window; every window that holds it is in workgroup 0
        assert bps == (1 if n_win == 96 else 2) and (value < 65504) == (value == 1e4)
