"""Every build of the staged-frame window kernels behind rp_mlp_forward_windows -- mlp_windows_kernel<NT, P3>, NT 1..7, and
mlp_windows_wide_kernel<NT, NQ, P3>, NT 2 / 4, NQ 2..5, each in three bf16 parts and in two f16 parts -- on the case table of
tests/mlp_windows_cases.py, whose coverage tests/test_mlp_windows_cases.py proves without a GPU:
 (a) every case runs the kernel the restated route names and gives the f64 reference's logits within the project's gate, the same bytes on
     a second call and for a stream alone; the route edges leave the staged-frame kernels as named;
 (b) the rows of a workgroup are, bit for bit, what its frames give as a stream of their own -- the restated cut against the device's, and
     one build against another (the 97-row tail of 257 windows under NT 5 against NT 4 alone, wide NT 4 against NT 2);
 (c) every partial product of a form is present: streams and weights whose parts are as large as parts get, nothing cancelling, against
     ((16 L + 8) 2^-24 + t) sum|x||w| with t derived from the splits (mlp_windows_cases.py says which missing products that gate can show);
 (d) a large frame INSIDE the workgroup's middle window, whose mean every frame of the workgroup is staged relative to: the windows that
     hold it keep the gate of (a); the other windows of the workgroup keep it with the scale widened to |mu - c|; the neighbouring workgroup
     and the other stream keep their bytes;
 (e) RP_MLP_WIN_TILES (read once per process) in child processes: the capped cut gives the same logits and the same slice identity.
Each test prints its worst error over gate; profiles/mlp_windows_builds.txt keeps those lines as measured."""
import numpy as np
import pytest

import child_runs
import mlp_windows_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


@pytest.fixture(scope="module")
def model(ra, ctx):
    made = {}

    def get(ws, bs):
        key = tuple(id(w) for w in ws)
        if key not in made:
            made[key] = (ra.Model(ctx, list(ws), list(bs)), ws)      # (ws is kept alive beside the handle: ids stay unique)
        return made[key][0]
    return get


def _report(what, case, shape, worst):
    print("mlp_windows_builds: %-7s %-34s NT %d NQ %d workgroups %d last %3d rows: worst err / gate %.4f" % ((what, case) + tuple(shape) + (worst,)))


# ------------------------------------------------------------------ (a)
@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_every_build_matches_the_f64_reference(ctx, model, case):
    L, prec = case[0], case[4]
    mfcc, ws, bs = M.inputs_of(case)
    name, nt, nq, bps, last = M.route_of(case)
    md = model(ws, bs)
    got = ctx.mlp_forward_windows(mfcc, md, precision=prec)
    assert ctx.last_mlp_kernel() == name
    ref = M.reference_of(case)
    assert got.shape == ref.shape and np.isfinite(got).all()
    gate = M.gate(ref, mfcc, L)
    worst = float((np.abs(got - ref) / gate).max())
    _report("f64", M.case_id(case), (nt, nq, bps, last), worst)
    assert worst <= 1.0, worst
    assert (np.abs(got - M.oracle(mfcc, L, ws, bs)) <= 1.25 * gate).all()      # the second witness, itself within a quarter of the gate
    assert ctx.mlp_forward_windows(mfcc, md, precision=prec).tobytes() == got.tobytes()
    S = mfcc.shape[0]
    assert ctx.mlp_forward_windows(mfcc[S - 1:], md, precision=prec).tobytes() == got[S - 1:].tobytes()


@pytest.mark.parametrize("edge", M.EDGES, ids=M.case_id)
def test_route_edges_leave_the_staged_frame_kernels(ctx, model, edge):
    """one frame beyond the longest window, layer 1 beyond 144, a tail layer of 33, 31 windows, another mfcc size: mlp_mfma_kernel reading
    the windows in place, or the per-layer kernel (which leaves the name as it was) -- and the reference's logits either way"""
    L, prec = edge[0], edge[4]
    mfcc, ws, bs = M.inputs_of(edge)
    name = M.route_of(edge)[0]
    md = model(ws, bs)
    before = ctx.last_mlp_kernel()
    got = ctx.mlp_forward_windows(mfcc, md, precision=prec)
    assert ctx.last_mlp_kernel() == (before if name is None else name)
    ref = M.reference_of(edge)
    worst = float((np.abs(got - ref) / M.gate(ref, mfcc, L)).max())
    _report("edge", M.case_id(edge), (0, 0, 0, 0), worst)
    assert got.shape == ref.shape and np.isfinite(got).all() and worst <= 1.0, worst


# ------------------------------------------------------------------ (b)
@pytest.mark.parametrize("case", M.MULTI, ids=M.case_id)
def test_a_workgroup_has_the_bits_of_its_slice(ctx, model, case):
    """rows [w0, w0 + rows) of the whole run against frames [w0, w0 + rows + L - 1) run as a stream of their own, byte for byte, for every
    workgroup of at least 32 rows (fewer take mlp_mfma_kernel alone): the frames, their middle window and the order of every sum are the
    same, whichever build of the kernel the slice's own window count selects"""
    L, prec = case[0], case[4]
    mfcc, ws, bs = M.inputs_of(case)
    name, nt, nq, bps, last = M.route_of(case)
    md = model(ws, bs)
    whole = ctx.mlp_forward_windows(mfcc, md, precision=prec)
    assert ctx.last_mlp_kernel() == name
    wgs = M.workgroups(case[3], nt)
    assert len(wgs) == bps and wgs[-1][1] == last
    met = set()
    for w0, rows in wgs:
        if rows < 32:
            continue
        alone = ctx.mlp_forward_windows(np.ascontiguousarray(mfcc[:, w0:w0 + rows + L - 1]), md, precision=prec)
        assert ctx.last_mlp_kernel() == name
        snt, _, sbps, _ = M.route(M.dims_of(case), 16, rows, prec)[1:]
        assert sbps == 1 and alone.shape == (mfcc.shape[0], rows, case[2])
        assert alone.tobytes() == whole[:, w0:w0 + rows].tobytes(), (w0, rows, nt, snt)
        met.add(snt)
    print("mlp_windows_builds: slices  %-34s NT %d NQ %d against NT %s alone: equal bytes" % (M.case_id(case), nt, nq, sorted(met)))
    assert met


# ------------------------------------------------------------------ (c)
@pytest.mark.parametrize("d1,n_win,prec,pattern", M.PARTS_CASES)
def test_every_partial_product_is_present(ra, ctx, d1, n_win, prec, pattern):
    mfcc, ws, bs = M.parts_inputs(d1, n_win, pattern)
    md = ra.Model(ctx, list(ws), list(bs))
    got = ctx.mlp_forward_windows(mfcc, md, precision=prec)
    name, nt, nq, bps, last = M.route((16 * M.PARTS_L, d1), 16, n_win, prec)
    assert ctx.last_mlp_kernel() == name and name.startswith("mlp_windows_")
    ref = M.reference(mfcc, M.PARTS_L, ws, bs)
    assert got.shape == ref.shape and np.isfinite(got).all()
    ratio = np.abs(got - ref) / M.parts_gate(mfcc, ws, prec)
    worst = float(ratio.max())
    _report("parts", "d1 %d %s weights '%s'" % (d1, prec, pattern), (nt, nq, bps, last), worst)
    assert worst <= 1.0, (worst, np.unravel_index(ratio.argmax(), ratio.shape))


# ------------------------------------------------------------------ (d)
@pytest.mark.parametrize("hidden,n_win,prec,value", M.HOT_CASES)
def test_a_large_frame_inside_the_middle_window(ctx, model, hidden, n_win, prec, value):
    """Every frame of a workgroup is staged minus c, the mean of its middle window.  A large frame inside that window moves c by value / L
    in one coefficient; every window of the workgroup that does not hold the frame then carries staged values of that size, which the
    correction -(mu - c) . wsum takes out again: its logits stay right to 1e-5 of |mu - c| (the widened scale below), not of the window's
    own features.  The windows that hold the frame keep the gate of (a) -- in the two-part form, beyond the f16 range, from the f32 pass --
    and the damage stops at the workgroup: its neighbour and the other stream keep the clean run's bytes."""
    L, S = M.HOT_L, 2
    dims = (16 * L,) + hidden + (2,)
    ws, bs = M.model_of(dims)
    md = model(ws, bs)
    name, nt, nq, bps, last = M.route(dims, 16, n_win, prec)
    clean_in = M.streams(S, n_win + L - 1, 16, ("hot", hidden, n_win))
    clean = ctx.mlp_forward_windows(clean_in, md, precision=prec)
    hot_in = clean_in.copy()
    frame = M.hot_frame(n_win, nt)
    hot_in[1, frame, 5] = value
    got = ctx.mlp_forward_windows(hot_in, md, precision=prec)
    assert ctx.last_mlp_kernel() == name and name.startswith("mlp_windows_")
    assert got.shape == clean.shape and np.isfinite(got).all()
    w0, rows = M.workgroups(n_win, nt)[0]
    inside = np.zeros(n_win, bool)
    inside[max(frame - L + 1, 0):frame + 1] = True
    here = np.zeros(n_win, bool)
    here[w0:w0 + rows] = True
    assert inside.sum() == L and (here | ~inside).all()
    # the other stream and the neighbouring workgroup: the clean run's bytes
    assert got[0].tobytes() == clean[0].tobytes() and got[1, ~here].tobytes() == clean[1, ~here].tobytes()
    assert (bps > 1) == (n_win == 225) and (~here).any() == (bps > 1)
    ref = M.reference(hot_in, L, ws, bs)
    err = np.abs(got - ref)
    # windows that hold the frame: the gate of (a), whose scale is the largest centred feature -- the frame itself
    gate = M.gate(ref, hot_in, L)
    assert M.spread(hot_in, L) >= 0.9 * value
    worst_in = float((err[1, inside] / gate[1, inside]).max())
    # the other windows of the workgroup: the scale widened to max_k |mu_row[k] - c[k]|, c recomputed from the restated cut
    mu = M.window_means(hot_in[1], L)
    c = mu[w0 + rows // 2]
    assert abs(c[5] - mu[0][5]) >= 0.9 * value / L
    other = here & ~inside
    scale = np.maximum(np.maximum(np.abs(ref[1, other]), M.spread(clean_in, L)), np.abs(mu[other] - c).max(axis=1, keepdims=True))
    worst_out = float((err[1, other] / (1e-5 * scale)).max())
    _report("hot in", "%s %s %g" % ("x".join(map(str, hidden)), prec, value), (nt, nq, bps, last), worst_in)
    _report("hot out", "%s %s %g" % ("x".join(map(str, hidden)), prec, value), (nt, nq, bps, last), worst_out)
    assert worst_in <= 1.0 and worst_out <= 1.0, (worst_in, worst_out)
    assert not np.array_equal(got[1, other], clean[1, other])            # they did see another c
    # nothing of this depends on what else the call holds or lists: the stream alone, and the call again, give the same bytes
    assert ctx.mlp_forward_windows(hot_in[1:], md, precision=prec).tobytes() == got[1:].tobytes()
    assert ctx.mlp_forward_windows(hot_in, md, precision=prec).tobytes() == got.tobytes()
    both = hot_in.copy()
    both[0, frame + 3, 2] = -value           # the other stream lists windows of its own (two parts, 1e6): this stream's rows do not move
    assert ctx.mlp_forward_windows(both, md, precision=prec)[1].tobytes() == got[1].tobytes()


# ------------------------------------------------------------------ (e)
_CHILD = """
import mlp_windows_cases as M
out = {}
for prec in M.PRECISIONS:
    case = (20, (32, 16), 2, 225, prec)
    mfcc, ws, bs = M.inputs_of(case)
    out[prec] = ctx.mlp_forward_windows(mfcc, ra.Model(ctx, list(ws), list(bs)), precision=prec)
    out["name_" + prec] = np.array(ctx.last_mlp_kernel())
np.savez(sys.argv[1], **out)
"""


def test_the_tile_cap_of_a_process(tmp_path, ctx, model):
    """RP_MLP_WIN_TILES 3 and 6 on 225 windows (three workgroups of three tiles -- 96, 96 and 33 rows -- and two of four): the child's logits
    keep the gate of (a), and each of its workgroups has the bits of its slice run here, under this process's cap of 7"""
    runs = child_runs.run_each(tmp_path, _CHILD, [("cap3", {"RP_MLP_WIN_TILES": "3"}), ("cap6", {"RP_MLP_WIN_TILES": "6"})], timeout=60)
    for cap, key in ((3, "cap3"), (6, "cap6")):
        for prec in M.PRECISIONS:
            case = (20, (32, 16), 2, 225, prec)
            assert case in M.CASES
            mfcc, ws, bs = M.inputs_of(case)
            got = runs[key][prec]
            name, nt, nq, bps, last = M.route_of(case, cap=cap)
            assert str(runs[key]["name_" + prec]) == name and (nt, bps) == M.cut(225, cap)
            ref = M.reference_of(case)
            worst = float((np.abs(got - ref) / M.gate(ref, mfcc, 20)).max())
            _report("cap %d" % cap, M.case_id(case), (nt, nq, bps, last), worst)
            assert got.shape == ref.shape and np.isfinite(got).all() and worst <= 1.0, worst
            for w0, rows in M.workgroups(225, nt):
                assert rows >= 32
                alone = ctx.mlp_forward_windows(np.ascontiguousarray(mfcc[:, w0:w0 + rows + 19]), model(ws, bs), precision=prec)
                assert alone.tobytes() == got[:, w0:w0 + rows].tobytes(), (cap, prec, w0, rows)
