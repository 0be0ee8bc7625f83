"""mlp_stream_kernel's walk (rp_mlp_stream.hip) at every row length class, base phase, build and tile count that
tests/mlp_stream_cases.py lists (its coverage is proven on the CPU by tests/test_mlp_stream_cases.py): integer models that every arithmetic
must return exactly, N(0, 1) models against the oracle, batch edges, the builds behind RP_MLP_STREAM_DEPTH / RP_MLP_STREAM_WAVES named by
rp_ctx_last_mlp_kernel, several tiles per workgroup, and the distance from an f64 forward held against the oracle's own.

Rows go in by device pointer at float offset 4 * q0 of a torch buffer (512-byte aligned) whose slack is NaN: the kernel reads whole 128-byte
lines from below the first row to behind the last one, and none of that may reach a result."""
import numpy as np
import pytest

import mlp_stream_cases as M

pytestmark = pytest.mark.gpu

KNOB_VARS = ("RP_MLP_STREAM", "RP_MLP_STREAM_DEPTH", "RP_MLP_STREAM_WAVES")


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def dctx(ra):
    import torch
    c = ra.BatchContext(0, host_pointers=False)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


@pytest.fixture(scope="module")
def models(ra, dctx):
    """ra.Model of (kind, row length, index into MODELS), made once"""
    made = {}

    def get(kind, n, mi):
        if (kind, n, mi) not in made:
            ws, bs = (M.integer_model if kind == "int" else M.random_model)(n, mi)
            made[kind, n, mi] = ra.Model(dctx, list(ws), list(bs))
        return made[kind, n, mi]
    return get


@pytest.fixture(scope="module")
def on_device():
    """the rows of a test on the device, uploaded once per array"""
    import torch
    held = {}

    def get(x):
        key = (x.ctypes.data, x.shape)
        if key not in held:
            held[key] = (x, torch.from_numpy(x.reshape(-1).copy()).cuda())   # (x itself: keeps the address taken)
        return held[key][1]
    return get


def _knobs(monkeypatch, prec, knob=None):
    """the launch knobs of one forward: RP_MLP_STREAM=2 where strict f32 is to stream (by default it takes mlp_mfma_kernel), nothing else
    unless the test asks for it"""
    for v in KNOB_VARS:
        monkeypatch.delenv(v, raising=False)
    if prec == "f32_strict":
        monkeypatch.setenv("RP_MLP_STREAM", "2")
    for k, v in (knob or {}).items():
        monkeypatch.setenv(k, v)


def _forward(dctx, model, xd, B, n, q0, prec, n_out, report):
    """logits of B rows of n floats held in device tensor xd, sent from a base q0 chunks into a 128-byte line, NaN before and behind"""
    import torch
    off = 4 * q0
    buf = torch.full((off + B * n + 64,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 128 == 0
    buf[off:off + B * n] = xd
    out = torch.full((B, n_out), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # torch's default stream is "the context's own stream" to rp_ctx_set_stream: order by hand
    dctx.mlp_dev(model, buf.data_ptr() + 4 * off, B, prec, out.data_ptr())
    dctx.synchronize()
    got = dctx.last_mlp_kernel()
    if report.startswith("mlp_mfma_kernel"):   # a model mlp_stream_kernel has no room for (mlp_stream_cases.TWIN): said, not assumed
        assert got.startswith(report) and "mlp_stream_kernel" not in got, (got, report)
    else:
        assert "mlp_stream_kernel" in got and got == report, (got, report)
    return out.cpu().numpy()


def _run(dctx, models, on_device, kind, n, mi, x, q0, prec, report=None):
    dims = M.dims_of(n, M.MODELS[mi])
    return _forward(dctx, models(kind, n, mi), on_device(x), x.shape[0], n, q0, prec, dims[-1],
                    M.stream_report(dims, prec, {}) if report is None else report)


def _turns(n, shift=0, arith=M.ARITH):
    """((index, arithmetic), model) for rows of n floats: the rotation of mlp_stream_cases.models_for"""
    return [((a, prec), mi) for a, prec in enumerate(arith) for mi in M.models_for(n, a, shift)]


# ------------------------------------------------------------------ every case x every arithmetic
@pytest.mark.parametrize("n", M.INS)
def test_every_case_every_arithmetic_exact(dctx, models, on_device, monkeypatch, n):
    """integer models (every partial sum below 2^24): f32 (three bf16 parts), f32_fast (two f16 parts), f32_strict and bf16 all return the
    f64 integers, at every base phase of the case list, finite despite the NaN slack -- and so the same bits at every phase"""
    x = M.integer_rows(n, M.B_CASES)
    q0s = [q for m, q in M.CASES if m == n]
    assert q0s
    for (a, prec), mi in _turns(n):
        want = M.integer_logits(n, mi, M.B_CASES)
        _knobs(monkeypatch, prec)
        outs = [_run(dctx, models, on_device, "int", n, mi, x, q0, prec) for q0 in q0s]
        for q0, o in zip(q0s, outs):
            assert np.isfinite(o).all(), (prec, q0)
            assert np.array_equal(o, want), (prec, q0, M.MODELS[mi], np.abs(o - want).max(), np.argwhere(o != want)[:4])
            assert o.tobytes() == outs[0].tobytes(), (prec, q0)


@pytest.mark.parametrize("n", M.INS)
def test_every_case_random_models(dctx, models, on_device, monkeypatch, n):
    """N(0, 1) models at the same cases: within the project's 1e-5 + 1e-5 |ref| of the oracle (bf16: 1e-3 of the bf16-rounding oracle), the
    same bits on a second call and at every base phase"""
    x = M.random_rows(n, M.B_CASES)
    q0s = [q for m, q in M.CASES if m == n]
    for (a, prec), mi in _turns(n):
        ref = M.oracle_logits(n, mi, M.B_CASES, bf16=prec == "bf16")
        tol = 1e-3 if prec == "bf16" else 1e-5
        _knobs(monkeypatch, prec)
        outs = [_run(dctx, models, on_device, "rnd", n, mi, x, q0, prec) for q0 in q0s]
        for q0, o in zip(q0s, outs):
            assert np.isfinite(o).all(), (prec, q0)
            assert np.allclose(o, ref, rtol=tol, atol=tol), (prec, q0, M.MODELS[mi], np.abs(o - ref).max())
            assert o.tobytes() == outs[0].tobytes(), (prec, q0)
        again = _run(dctx, models, on_device, "rnd", n, mi, x, q0s[-1], prec)
        assert again.tobytes() == outs[-1].tobytes(), prec


@pytest.mark.parametrize("n", M.INS)
def test_every_case_nan_row_stays_in_its_row(dctx, models, on_device, monkeypatch, n):
    """a row's lines also hold the end of the row before it and the start of the one behind it (and the array's last lines are clamped onto
    its last bytes, so the NaN slack alone never shows this): NaN in the first and the last feature of rows 17 and B - 1 makes those rows'
    logits NaN and leaves every other row exact, at every phase and in every arithmetic"""
    B = M.B_CASES
    x = M.integer_rows(n, B).copy()
    hot = [17, B - 1]
    for r in hot:
        x[r, 0] = x[r, n - 1] = np.nan
    q0s = [q for m, q in M.CASES if m == n]
    for (a, prec), mi in _turns(n):
        want = np.delete(M.integer_logits(n, mi, B), hot, axis=0)
        _knobs(monkeypatch, prec)
        for q0 in q0s:
            o = _run(dctx, models, on_device, "int", n, mi, x, q0, prec)
            assert np.isnan(o[hot]).all(), (prec, q0)
            assert np.array_equal(np.delete(o, hot, axis=0), want), (prec, q0, M.MODELS[mi])


# ------------------------------------------------------------------ batch edges
@pytest.mark.parametrize("n", [96, 80])
@pytest.mark.parametrize("B", [1, 2, 16, 17, 127, 128, 129, 255, 256, 257])
def test_batch_edges_exact_and_position_independent(dctx, models, on_device, monkeypatch, n, B):
    """batches around a wave's 16 rows and a workgroup tile's 128 (256 of one parity when par = 1): exact, and rows 1.. sent alone (odd rows
    become even ones, the last tile ends elsewhere) keep their bits"""
    full = M.integer_rows(n, 257, 1)
    x, x1 = np.ascontiguousarray(full[:B]), np.ascontiguousarray(full[1:B])
    for (a, prec), mi in _turns(n):
        want = M.integer_logits(n, mi, 257, 1)[:B]
        _knobs(monkeypatch, prec)
        o = _run(dctx, models, on_device, "int", n, mi, x, 0, prec)
        assert np.array_equal(o, want), (prec, np.argwhere(o != want)[:4])
        if B > 1:
            o1 = _run(dctx, models, on_device, "int", n, mi, x1, 0, prec)
            assert o1.tobytes() == o[1:].tobytes(), prec


# ------------------------------------------------------------------ builds
@pytest.mark.parametrize("knob", M.KNOBS, ids=lambda k: "-".join("%s=%s" % (a[len("RP_MLP_STREAM_"):], b) for a, b in k.items()) or "default")
@pytest.mark.parametrize("n", M.BUILD_INS)
def test_builds_same_bits_and_named(dctx, models, on_device, monkeypatch, n, knob):
    """RP_MLP_STREAM_DEPTH=1, RP_MLP_STREAM_WAVES=4 and =6 (f32 callers): other template builds of one arithmetic -- nothing in a row's chain of
    sums depends on the ring depth or on the waves of a workgroup, so the bits are the default build's.  rp_ctx_last_mlp_kernel names the
    build where a knob moved it, and only there: a knob the LDS conditions refuse leaves the default build and the plain report."""
    xi, xr = M.integer_rows(n, M.B_CASES), M.random_rows(n, M.B_CASES)
    for mi in M.BUILD_MODELS:
        dims = M.dims_of(n, M.MODELS[mi])
        for prec in M.ARITH:
            if "RP_MLP_STREAM_WAVES" in knob and knob["RP_MLP_STREAM_WAVES"] == "6" and prec != "f32":
                continue   # the knob applies to the three-part form alone (test_mlp_stream_cases.py holds the launcher's table to that)
            for q0 in M.BUILD_Q0S:
                _knobs(monkeypatch, prec)
                base_i = _run(dctx, models, on_device, "int", n, mi, xi, q0, prec)
                base_r = _run(dctx, models, on_device, "rnd", n, mi, xr, q0, prec)
                _knobs(monkeypatch, prec, knob)
                rep = M.stream_report(dims, prec, knob)
                got_i = _run(dctx, models, on_device, "int", n, mi, xi, q0, prec, rep)
                got_r = _run(dctx, models, on_device, "rnd", n, mi, xr, q0, prec, rep)
                assert np.array_equal(got_i, M.integer_logits(n, mi, M.B_CASES)), (dims, prec, q0)
                assert got_i.tobytes() == base_i.tobytes() and got_r.tobytes() == base_r.tobytes(), (dims, prec, q0)
                tol = 1e-3 if prec == "bf16" else 1e-5
                assert np.allclose(got_r, M.oracle_logits(n, mi, M.B_CASES, bf16=prec == "bf16"), rtol=tol, atol=tol), (dims, prec, q0)


# ------------------------------------------------------------------ several tiles per workgroup
def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("n,waves", [(64, 8), (64, 4), (80, 8)])
@pytest.mark.parametrize("q0", [0, 5])
def test_several_tiles_per_workgroup_exact(dctx, models, on_device, monkeypatch, n, waves, q0):
    """more tiles than workgroups (three on the first workgroups, two elsewhere, a ragged last one; twice that on the four-wave build): the
    DMA stream runs on into the next tile while the last one is worked on, the phase is chosen again per tile, the sums start from zero --
    every row of an integer model is exact in every arithmetic"""
    n_cu = _n_cu()
    B = M.multi_tile_B(n, n_cu, waves)
    x = M.integer_rows(n, B, 2)
    knob = {"RP_MLP_STREAM_WAVES": "4"} if waves == 4 else {}
    for (a, prec), mi in _turns(n, 0 if waves == 4 else 5):
        dims = M.dims_of(n, M.MODELS[mi])
        if waves == 4:
            assert M.stream_build(dims, prec, knob)[:2] == (1, 4)
        _knobs(monkeypatch, prec, knob)
        o = _run(dctx, models, on_device, "int", n, mi, x, q0, prec, M.stream_report(dims, prec, knob))
        want = M.integer_logits(n, mi, B, 2)
        assert np.array_equal(o, want), (prec, M.MODELS[mi], np.argwhere(o != want)[:4])


@pytest.mark.parametrize("n", [64, 80])
@pytest.mark.parametrize("q0", [0, 5])
def test_several_tiles_per_workgroup_random_and_out_of_range_rows(dctx, models, on_device, monkeypatch, n, q0):
    """N(0, 1) models across tile boundaries: rows of a workgroup's first, second and third tile carry the bits they have in a small batch
    of their own (f32, f32_fast); and a feature beyond the f16 range in a row of a workgroup's FIRST tile and in the batch's last row sends
    those two rows to the f32 matrix instructions (their f32_strict bits) and no other -- the range a lane has seen is forgotten per tile"""
    n_cu = _n_cu()
    par = M.plan(n, 0)["par"]
    B = M.multi_tile_B(n, n_cu)
    x = M.random_rows(n, B, 2)
    rows = M.multi_tile_sample(B, par, n_cu)
    xs = np.ascontiguousarray(x[rows])
    plain = {}
    for (a, prec), mi in _turns(n, 5, M.ARITH[:2]):
        _knobs(monkeypatch, prec)
        o = plain[prec, mi] = _run(dctx, models, on_device, "rnd", n, mi, x, q0, prec)
        small = _run(dctx, models, on_device, "rnd", n, mi, xs, q0, prec)
        assert np.isfinite(o).all() and o[rows].tobytes() == small.tobytes(), prec
        ref = M.oracle_logits(n, mi, B, seed=2)
        assert np.allclose(o, ref, rtol=1e-5, atol=1e-5), (prec, np.abs(o - ref).max())
    mi = M.models_for(n, 1, 5)[-1]
    assert M.stream_supported(M.dims_of(n, M.MODELS[mi]), "f32_fast")
    hot = [3, B - 1]
    assert M.row_tile(3, par) < n_cu   # a first tile; its workgroup goes on to a second one
    xb = x.copy()
    xb[3, 7] = 7.0e4
    xb[B - 1, n - 1] = -7.0e4
    _knobs(monkeypatch, "f32_fast")
    big = _run(dctx, models, on_device, "rnd", n, mi, xb, q0, "f32_fast")
    _knobs(monkeypatch, "f32_strict")
    strict = _run(dctx, models, on_device, "rnd", n, mi, xb, q0, "f32_strict")
    assert np.isfinite(big).all()
    assert big[hot].tobytes() == strict[hot].tobytes()
    assert np.delete(big, hot, axis=0).tobytes() == np.delete(plain["f32_fast", mi], hot, axis=0).tobytes()


# ------------------------------------------------------------------ distance from f64
@pytest.mark.parametrize("n", [64, 1040, 3120])
def test_distance_from_f64_no_worse_than_the_oracle(dctx, models, on_device, monkeypatch, n, capsys):
    """single-layer N(0, 1) model (32 outputs): e = |logit - f64 logit| over S = |x| @ |w|.T, in units of 2^-24.  The reference is the
    oracle's own maximum (an f32 sequential sum: 3.7 to 4.3 units on such data); each kernel form's maximum must stay within 1.25 of it
    (the margin of tests/test_gpu_model_pin.py).  Measured values: profiles/mlp_stream_edges.txt."""
    mi = M.MODELS.index((32, ()))
    ws, bs = M.random_model(n, mi)
    x = M.random_rows(n, M.B_CASES)
    tru = M.f64_forward(x, ws, bs)
    S = np.abs(x.astype(np.float64)) @ np.abs(ws[0].astype(np.float64)).T
    unit = lambda got: float((np.abs(got.astype(np.float64) - tru) / S).max() * 2.0 ** 24)
    e = {"oracle": unit(M.oracle_logits(n, mi, M.B_CASES))}
    for prec in M.ARITH[:3]:
        _knobs(monkeypatch, prec)
        e[prec] = unit(_run(dctx, models, on_device, "rnd", n, mi, x, 0, prec))
    with capsys.disabled():
        print("\nmlp_stream_kernel e/S max, units of 2^-24, in = %d: " % n + ", ".join("%s %.3f" % kv for kv in e.items()))
    assert 1.0 < e["oracle"] < 8.0, e   # the premise: an f32-grade evaluation, as measured on the CPU
    for prec in M.ARITH[:3]:
        assert e[prec] <= 1.25 * e["oracle"], (prec, e)
