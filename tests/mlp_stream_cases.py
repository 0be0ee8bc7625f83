"""What the tests of mlp_stream_kernel's walk share (tests/test_mlp_stream_cases.py on the CPU, tests/test_gpu_mlp_stream_edges.py on the GPU):
a restatement of Model::stream_plan's integers (rp_ctx.cpp) and of launch_mlp_stream's choice of build (rp_mlp_stream.hip), the list of
(row length, base phase) cases, the models and the two references.

The walk of a row is decided by (in, q0), q0 = the 16-byte chunks between the array's base and the 128-byte line below it:
  par    1 when the row pitch is an odd number of half lines: odd rows start four chunks further into a line than even ones (q1);
  lines  the 128-byte lines that hold bytes of a row at the larger of the two phases; units = lines rounded up to pairs;
  flush  the tile's last k-step 2 * units - 1 runs only when it still holds k below `in`;
  nx     per lane group lk = 0..3 and half: whether the lane's chunk of a k-step lies in the NEXT line (lk + 4 * half + q >= 8).
CASES crosses every class (par, flush, lines odd / even, units 1 / 2 / 3 and more) the formula can produce over INS x 0..7 with every q0 it
can occur at (50 classes: each phase is a different nx pattern meeting that class), plus the two long rows of the older tests.

References: (a) integer models -- features in [-8, 8], layer-1 weights in [-2, 2], small integer biases and tail weights: every partial sum
of every layer stays below 2^24, so bf16, the f16 pair, the bf16 triple, the f32 matrix instructions and the fmaf tails are all exact and
every arithmetic must return the f64 integers; (b) N(0, 1) models as in tests/test_gpu_mlp_stream.py, against the oracle and an f64 forward.
Everything returned from the caches is read-only."""
import functools

import numpy as np

F32 = np.float32
INS = (64, 80, 96, 112, 128, 144, 176, 1040, 3120)
ARITH = ("f32", "f32_fast", "f32_strict", "bf16")
# (layer-1 width, the layers behind it): single layers on both sides of the 16 / 17 tile boundary, a tail layer read in one round of 32 inputs
# (13: not a multiple of 4; 16) and in two (37, 100)
MODELS = ((1, ()), (16, ()), (17, ()), (32, ()), (13, (2,)), (32, (16, 2)), (17, (37, 3)), (32, (100, 5)), (1, (1,)), (16, (100, 5)))
# (32, (100, 5)) does not fit mlp_stream_kernel's LDS (eight waves' rows of 100 hidden values beside two 16-output tiles of weights:
# mlp_stream_supported refuses it and mlp_mfma_kernel serves it, which the tests assert rather than assume); wherever it is due, its
# one-tile twin (16, (100, 5)) runs as well, which does stream: four rounds of 32 inputs in the last layer
ROTATION = 9           # the models that take turns; the twin follows its sibling
TWIN = {7: 9}
B_CASES = 300
CASES = tuple([(n, q) for n in (64, 80, 96, 112, 128, 144) for q in range(8)] +
              [(176, 0), (176, 1), (176, 4), (1040, 0), (1040, 3), (3120, 0), (3120, 5)])


def plan(n, q0):
    """Model::stream_plan's integers for rows of n floats whose array starts q0 chunks into a line"""
    par = int((n // 4) % 8 != 0)
    q1 = (q0 + 4) & 7 if par else q0
    lines = (n - 1 + 4 * max(q0, q1)) // 32 + 1
    units = (lines + 1) // 2
    nx = {q: tuple((lk + q >= 8, lk + 4 + q >= 8) for lk in range(4)) for q in sorted({q0, q1})}
    return dict(par=par, q1=q1, lines=lines, units=units, flush=32 * (2 * units - 1) < n, nx=nx)


def plan_class(n, q0):
    p = plan(n, q0)
    return (p["par"], p["flush"], p["lines"] % 2, min(p["units"], 3), q0)


def dims_of(n, model):
    return (n, model[0]) + tuple(model[1])


def models_for(n, a, shift=0):
    """Which of MODELS (indices) rows of n floats meet in arithmetic ARITH[a]: over INS every model meets every arithmetic and both `par`
    values (test_mlp_stream_cases.py); chosen per (n, a), so that the phases of one row length are comparable bit for bit"""
    mi = (2 * INS.index(n) + a + shift) % ROTATION
    return (mi, TWIN[mi]) if mi in TWIN else (mi,)


def _frozen(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------ (a) integer models
@functools.lru_cache(maxsize=None)
def integer_model(n, mi):
    rng = np.random.default_rng(1000 * n + mi)
    dims = dims_of(n, MODELS[mi])
    ws, bs = [], []
    for l in range(len(dims) - 1):
        if l == 0:
            w = rng.integers(-2, 3, size=(dims[1], n))
        else:   # no zero: a one-input tail layer must not forget its input
            w = rng.choice(np.array([-2, -1, 1, 2]), size=(dims[l + 1], dims[l]))
        ws.append(_frozen(w.astype(F32)))
        bs.append(_frozen(rng.integers(-3, 4, size=dims[l + 1]).astype(F32)))
    return tuple(ws), tuple(bs)


@functools.lru_cache(maxsize=None)
def integer_rows(n, B, seed=0):
    return _frozen(np.random.default_rng(77 * n + B + seed).integers(-8, 9, size=(B, n)).astype(F32))


def f64_layers(x, ws, bs):
    """[(pre-activations, bound)] per layer in f64: bound = |input| @ |W|.T + |b|, above every partial sum in whatever order it is taken"""
    h = np.asarray(x, np.float64)
    out = []
    for l, (w, b) in enumerate(zip(ws, bs)):
        w, b = np.asarray(w, np.float64), np.asarray(b, np.float64)
        pre = h @ w.T + b
        out.append((pre, np.abs(h) @ np.abs(w).T + np.abs(b)))
        h = np.maximum(pre, 0.0) if l + 1 < len(ws) else pre
    return out


def f64_forward(x, ws, bs):
    return f64_layers(x, ws, bs)[-1][0]


@functools.lru_cache(maxsize=None)
def integer_logits(n, mi, B, seed=0):
    ws, bs = integer_model(n, mi)
    layers = f64_layers(integer_rows(n, B, seed), ws, bs)
    assert max(bound.max() for _, bound in layers) < 2 ** 24   # the premise, for these very rows: integers below 2^24 are exact in f32
    return _frozen(layers[-1][0].astype(F32))


def integer_model_worst_case(n, mi):
    """the largest sum of magnitudes any row of features in [-8, 8] can reach in any layer of integer_model(n, mi)"""
    ws, bs = integer_model(n, mi)
    h, worst = np.full(n, 8.0), 0.0
    for w, b in zip(ws, bs):
        h = np.abs(w.astype(np.float64)) @ h + np.abs(b.astype(np.float64))
        worst = max(worst, float(h.max()))
    return worst


# ------------------------------------------------------------------ (b) N(0, 1) models
@functools.lru_cache(maxsize=None)
def random_model(n, mi):
    rng = np.random.default_rng(5000 * n + mi)
    dims = dims_of(n, MODELS[mi])
    ws = tuple(_frozen((rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(F32)) for i in range(len(dims) - 1))
    bs = tuple(_frozen((rng.standard_normal(dims[i + 1]) * 0.1).astype(F32)) for i in range(len(dims) - 1))
    return ws, bs


@functools.lru_cache(maxsize=None)
def random_rows(n, B, seed=0):
    return _frozen(np.random.default_rng(31 * n + B + seed).standard_normal((B, n)).astype(F32))


@functools.lru_cache(maxsize=None)
def oracle_logits(n, mi, B, bf16=False, seed=0):
    from oracle import rp_oracle as orc
    ws, bs = random_model(n, mi)
    return _frozen(orc.mlp_forward(random_rows(n, B, seed), list(ws), list(bs), bf16_layer1=bf16))


# ------------------------------------------------------------------ the builds (launch_mlp_stream)
FORM = {"f32": "bf16x3 splits", "f32_fast": "f16x2 splits", "f32_strict": "f32 matrix instructions", "bf16": "bf16"}
LISTED = " + mlp_mfma_kernel<f32> on listed rows"
KNOBS = ({}, {"RP_MLP_STREAM_DEPTH": "1"}, {"RP_MLP_STREAM_WAVES": "4"}, {"RP_MLP_STREAM_WAVES": "6"})
BUILD_MODELS = (4, 5, 3)   # of MODELS: one 16-output tile; two with tail layers (too much LDS for two four-wave workgroups); two without
BUILD_INS, BUILD_Q0S = (96, 1040), (0, 3)


def _pad4(n):
    return ((n + 3) & ~3) + 4


def stream_lds_bytes(dims, prec, depth, waves=8):
    """stream_lds_bytes over stream_tail_lds (rp_mlp_stream.hip) for a model of these dims"""
    nt, n_layers = (dims[1] + 15) // 16, len(dims) - 1
    tail, h2p = 0, 4
    for l in range(1, n_layers):
        tail += dims[l + 1] * _pad4(dims[l]) + ((dims[l + 1] + 3) & ~3)
        if l + 1 < n_layers:
            h2p = max(h2p, _pad4(dims[l + 1]))
    wu = {"bf16": 2048, "f32": 6144}.get(prec, 4096) * nt
    return (tail + 16 * nt) * 4 + (depth + 2) * wu + waves * (depth + 1) * 4096 + waves * 16 * (16 * nt + 4) * 4 + waves * 16 * h2p * 4


def stream_build(dims, prec, knob):
    """(ring depth, waves per workgroup) of the mlp_stream_kernel build launch_mlp_stream runs, and whether a knob moved it off the default"""
    cu_lds = 160 * 1024
    depth0 = 2 if stream_lds_bytes(dims, prec, 2) <= cu_lds else 1
    depth, waves = depth0, 8
    if knob.get("RP_MLP_STREAM_DEPTH") == "1":
        depth = 1
    w = knob.get("RP_MLP_STREAM_WAVES")
    if w == "4" and 2 * stream_lds_bytes(dims, prec, 1, 4) <= cu_lds:
        depth, waves = 1, 4
    if w == "6" and prec == "f32" and stream_lds_bytes(dims, prec, 2, 6) <= cu_lds:
        depth, waves = 2, 6
    return depth, waves, (depth, waves) != (depth0, 8)


def stream_supported(dims, prec):
    """mlp_stream_supported's LDS condition: the shallow ring of the three-part form, or of the f32 one for every other arithmetic"""
    return dims[1] <= 32 and dims[0] % 16 == 0 and dims[0] >= 64 and stream_lds_bytes(dims, "f32" if prec == "f32" else "f32_strict", 1) <= 160 * 1024


def stream_report(dims, prec, knob):
    """rp_ctx_last_mlp_kernel after a forward of 16-byte aligned dense rows: mlp_stream_kernel, its build named only where a knob moved it
    off the default; or the start of mlp_mfma_kernel's report for a model the streaming kernel has no room for"""
    if not stream_supported(dims, prec):
        return "mlp_mfma_kernel<"
    depth, waves, moved = stream_build(dims, prec, knob)
    return ("mlp_stream_kernel<" + FORM[prec] + ">" + (LISTED if prec == "f32_fast" else "") +
            (" [stream build: depth %d, %d waves]" % (depth, waves) if moved else ""))


# ------------------------------------------------------------------ tiles (launch_stream_t, tile_row0)
def row_tile(r, par, waves=8):
    """the workgroup tile that holds row r: 16 * waves rows, or the rows of one parity of a 32 * waves span"""
    return 2 * (r // (32 * waves)) + (r & 1) if par else r // (16 * waves)


def n_tiles(B, par, waves=8):
    return 2 * ((B + 32 * waves - 1) // (32 * waves)) if par else (B + 16 * waves - 1) // (16 * waves)


def multi_tile_B(n, n_cu, waves=8):
    """batches that give the first workgroups three tiles, the others two, and a ragged last tile; twice the rows for the
    four-wave build, whose tiles are half as large on twice as many workgroups"""
    B = 128 * (2 * n_cu + 1) + 77 if plan(n, 0)["par"] == 0 else 256 * n_cu + 300
    return B * (2 if waves == 4 else 1)


def multi_tile_sample(B, par, n_cu, waves=8, count=512, seed=3):
    """`count` rows of a multi-tile batch: row 0's workgroup's first, second and third tile in full or in part, the ragged last tile, the
    rest at random"""
    grid = min(n_tiles(B, par, waves), n_cu * (8 // waves))
    pick = set()
    span = 16 * waves * (2 if par else 1)
    for ordinal in range(3):
        bt = ordinal * grid   # workgroup 0's tile number `ordinal`
        r0 = (bt >> 1) * span if par else bt * span
        pick.update(range(r0, min(r0 + 40, B)))
        pick.update(range(max(r0 + span - 24, 0), min(r0 + span, B)))
    pick.update(range(B - 90, B))
    rng = np.random.default_rng(seed)
    while len(pick) < count:
        pick.add(int(rng.integers(0, B)))
    return np.array(sorted(pick))
