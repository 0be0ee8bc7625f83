"""What the tests of the staged-frame window kernels share (tests/test_mlp_windows_cases.py on the CPU, tests/test_gpu_mlp_windows_builds.py
on the GPU): a restatement of the cut of a stream's windows into workgroups (mlp_windows_cut, rp_mlp_dev.h:108-113), of the wide form's
2 / 4 tile rule (mlp_route, rp_mlp.hip:666-672) and of the route itself (Model::create, rp_ctx.cpp:773-803; mlp_route, rp_mlp.hip:641-698),
the table of cases that reaches each of the 30 builds of mlp_windows_kernel<NT, P3> (NT 1..7) and mlp_windows_wide_kernel<NT, NQ, P3>
(NT 2 / 4, NQ 2..5) in both arithmetics, the f64 reference, the project's logit gate, and an emulation of the kernels' product sets.

A case is (L, hidden, labels, n_win, precision): windows of L frames of 16 coefficients, layer widths `hidden` then `labels`, n_win windows per
stream, two streams (one for the 256-frame windows).  EDGES carry a sixth field, the mfcc size.

The partial-product cases (PARTS_*): single-layer models, L 8, streams that alternate +v, -v frame by frame.  Every |v[k]| has all 24
mantissa bits set and an exponent in [0.5, 4), so the truncating splits of the kernels give parts of the largest size a part can have
(three bf16 parts: 2^-8 and 2^-16 of x; two f16 parts: 2^-11 of x, and 2 bits of x are cut), and the column sums of every window are exactly 0
in frame order: mu = c = 0, the staged frames are the frames and the mean correction is 0.  sign(W[o][f][k]) = (-1)^f sign(v[k]): in every
window the 16 L terms of one product class x_i w_j carry one sign, so a class that went missing cannot hide behind cancellation.  Two
weight patterns: "ones", all mantissa bits set as the frames have -- which the HOST splits do not keep as large parts, for they round to
nearest: w0 = 2^(e+1), w1 = -2^(e-23), nothing behind it -- and "parts", the mantissa 1.1111111 0 11 0 11111 0 111111 whose rounded parts stay
near their largest (bf16: 2^-9 and 2^-18 of w; f16: 2^-12 of w).
The gate of those cases: |got - f64| <= ((16 L + 8) 2^-24 + t) sum|x||w|.  16 L + 8 roundings of half an f32 ulp of the sum of
magnitudes: one per term of the longest chain an f32 accumulation of a row can be, the three additions of the waves' partial sums, the mean
correction, the bias, and room for the matrix instruction's own order.  t is what the form leaves out by design, as a fraction of
sum|x||w|, computed from the splits of these very inputs (parts_truncation): three parts, the products x_i w_j with i + j >= 3 (about
1.5 2^-24); two parts, x1 w1, the two bits the frames' second part cuts and the rounding of the weights' second part (about 7 2^-24).
What a missing product does against that gate, L 8, (16 L + 8) 2^-24 = 2^-16.9: the first-order products (x1 w0, x0 w1 of either form; 2^-8
.. 2^-12 of the sum) miss it by 28x and more.  The second-order products of the three-part form CANNOT miss it by 8x whatever the inputs: a
third part is at most 2^-16 of its value, so x2 w0 missing is at most 256 2^-24 of sum|x||w| against a gate of 137.5 2^-24 (1.86x), x1 w1
128 2^-24 (0.9x), x0 w2 64 2^-24 (0.5x).  test_mlp_windows_cases.py asserts exactly these figures; a tighter gate would need the rounding
of a matrix instruction's internal sum, which is not documented."""
import functools
import zlib

import numpy as np

F32 = np.float32
K = 16
TILE, MAX_TILES = 32, 7
PRECISIONS = ("f32", "f32_fast")
FORM = {"f32": "bf16x3 splits", "bf16": "bf16x3 splits", "f32_strict": "f32 matrix instructions", "f32_fast": "f16x2 splits"}
LISTED = " + mlp_mfma_kernel<f32> on listed rows"


def _frozen(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------ the cut and the route
def cut(n_win, cap=MAX_TILES):
    """mlp_windows_cut: (tiles per workgroup, workgroups per stream) -- as few workgroups as `cap` tiles each allow, the tiles spread evenly"""
    tiles = (n_win + TILE - 1) // TILE
    if tiles == 0:
        return 0, 0
    wgs = (tiles + cap - 1) // cap
    per = (tiles + wgs - 1) // wgs
    return per, (n_win + per * TILE - 1) // (per * TILE)


def wide_cut(n_win):
    """the form-2 rule of mlp_route: four-tile workgroups, or one two-tile workgroup when that holds the stream"""
    tiles = (n_win + TILE - 1) // TILE
    wgs = (tiles + 3) // 4
    nt = 2 if (tiles + wgs - 1) // wgs <= 2 else 4
    return nt, (n_win + nt * TILE - 1) // (nt * TILE)


def workgroups(n_win, nt):
    """[(first window, rows)] of a stream cut into workgroups of nt tiles"""
    return [(w0, min(nt * TILE, n_win - w0)) for w0 in range(0, n_win, nt * TILE)]


def _mfma_lds(dims, nt, tail_floats, three):
    """mlp_mfma_lds (rp_mlp.hip:578-587) in bytes"""
    h2w = max([1] + [dims[l] + 1 for l in range(2, len(dims) - 1)]) | 1
    wbuf = max((24 if three else 16) * nt * 136 * (2 if nt <= 2 else 1), 8 * 16 * (16 * nt + 1))
    wbuf = (wbuf + 3) & ~3
    return (((tail_floats + 3) & ~3) + wbuf + 8 * 16 * h2w) * 4


def route(dims, k, n_win, precision, cap=MAX_TILES, windows_env=None):
    """(what rp_ctx_last_mlp_kernel prints after rp_mlp_forward_windows -- None: the per-layer kernel, which leaves the name as it was --,
    NT, NQ, workgroups per stream, rows of the last workgroup); NT = NQ = 0 off the staged-frame kernels.  dims: input, layer widths."""
    dims = tuple(dims)
    n_layers, n1 = len(dims) - 1, dims[1]
    assert 1 <= n_layers <= 3 and k % 4 == 0 and dims[0] % k == 0
    nt = 1 if n1 <= 16 else 2 if n1 <= 32 else 5 if n1 <= 80 else 9 if n1 <= 144 else 0      # Model::create
    tail_floats = sum(dims[l] * dims[l + 1] + dims[l + 1] for l in range(1, n_layers)) or 1
    ok = nt > 0 and dims[0] % 4 == 0 and all(dims[l] <= 255 for l in range(2, n_layers))
    if not ok or _mfma_lds(dims, nt, tail_floats, False) > 160 * 1024:
        return None, 0, 0, 0, 0
    form = 0
    if (precision != "f32_strict" and k == 16 and dims[0] % 16 == 0 and n_win >= 32 and 2 <= dims[0] // 16 <= 256 and tail_floats <= 6144
            and windows_env != "0"):
        form = 1 if n1 <= 32 else 2
        if any(d > 32 for d in dims[2:]):
            form = 0
    if form == 0:
        shape = FORM[precision]
        if shape == FORM["f32"] and _mfma_lds(dims, nt, tail_floats, True) > 160 * 1024:
            shape = FORM["f32_strict"]       # three-part weight groups beyond the LDS
        listed = "," + LISTED if precision == "f32_fast" else ""
        return "mlp_mfma_kernel<" + shape + ">, windows read in place" + listed, 0, 0, 0, 0
    tiles, bps = cut(n_win, cap) if form == 1 else wide_cut(n_win)
    name = ("mlp_windows_kernel<" if form == 1 else "mlp_windows_wide_kernel<") + FORM[precision] + ">" + (LISTED if precision == "f32_fast" else "")
    return name, tiles, (n1 + 31) // 32 if form == 2 else 0, bps, n_win - (bps - 1) * tiles * TILE


def dims_of(case, k=K):
    L, hidden, labels = case[0], case[1], case[2]
    return (L * k,) + tuple(hidden) + (labels,)


def route_of(case, **kw):
    return route(dims_of(case, case[5] if len(case) > 5 else K), case[5] if len(case) > 5 else K, case[3], case[4], **kw)


def build_of(case):
    """the kernel build a case runs: ("narrow" / "wide", NT, NQ, three parts?)"""
    name, nt, nq, _, _ = route_of(case)
    return ("wide" if nq else "narrow", nt, nq, case[4] == "f32")


ALL_BUILDS = frozenset([("narrow", nt, 0, p3) for nt in range(1, 8) for p3 in (True, False)] +
                       [("wide", nt, nq, p3) for nt in (2, 4) for nq in (2, 3, 4, 5) for p3 in (True, False)])


def streams_of(case):
    return 1 if case[0] == 256 else 2


# ------------------------------------------------------------------ the table
def _table():
    t = []
    # narrow, NT 1..7 with a last tile of one row and of 32 rows; the tail and the window length take turns
    for i, n_win in enumerate((32, 33, 65, 96, 97, 129, 161, 192, 193, 224, 64, 128, 160)):
        for prec in PRECISIONS:
            t.append(((8, 20)[i % 2], ((32, 16), (13,), (32, 32))[i % 3], 2, n_win, prec))
    # narrow, several workgroups: two of NT 4; NT 5 whose last workgroup (97 rows) has a wholly empty fifth tile; NT 6 x 2; NT 7 x 2;
    # NT 5 x 3; NT 6 x 4 with 97 rows in the last
    for i, n_win in enumerate((225, 257, 353, 417, 449, 673)):
        for prec in PRECISIONS:
            t.append(((20, 8)[i % 2], (32, 16), 2, n_win, prec))
    # wide: NQ 2..5, NT 2 (33, 64), NT 4 with an empty fourth tile (65), full (128), a second and a third workgroup of one row (129, 257),
    # and second workgroups of 33 and 64 rows, which alone are the NT 2 build (161, 192)
    for q, d1 in enumerate((33, 65, 97, 129)):
        for i, n_win in enumerate((33, 64, 65, 128, 129, 257, 161, 192)):
            for prec in PRECISIONS:
                t.append(((8, 20)[(i + q) % 2], ((d1, 32), (d1,), (d1, 31))[(i + q) % 3], 2 if (i + q) % 3 else 4, n_win, prec))
    # layer-1 widths on both sides of every tile edge
    for i, d1 in enumerate((64, 96, 128, 144)):
        t.append((8, (d1, 16), 2, 97, PRECISIONS[i % 2]))
    for i, d1 in enumerate((1, 16, 17, 32)):
        t.append((8, (d1, 5), 2, 97, PRECISIONS[i % 2]))
    # depth and width: one, two and three layers, odd tail widths, 1 / 2 / 32 labels
    for i, (hidden, labels) in enumerate((((), 1), ((), 32), ((32,), 1), ((20, 1), 2), ((32, 3), 32), ((31, 32), 32), ((40,), 32), ((65, 1), 1),
                                          ((), 40), ((100, 32, ), 1), ((129, 3), 2))):
        t.append((8, hidden, labels, 70, PRECISIONS[i % 2]))
    # window lengths: waves of the narrow kernel that own no frames (L < 4), the weight prefetch clamped at once (L < 3), the longest window.
    # L 1: every normalised feature is 0 -- mlp_route keeps such windows with mlp_mfma_kernel, which the test of the table asserts
    for i, L in enumerate((1, 2, 3, 4, 5, 13)):
        for prec in PRECISIONS:
            t.append((L, (32, 16), 2, 65, prec))
        t.append((L, (65, 32), 2, 65, PRECISIONS[i % 2]))
    for prec in PRECISIONS:
        t.append((256, (32, 16), 2, 224, prec))
        t.append((256, (65, 32), 2, 128, prec))
    assert len(set(t)) == len(t)
    return tuple(t)


CASES = _table()
MULTI = tuple(c for c in CASES if route_of(c)[3] > 1)
# route edges (L, hidden, labels, n_win, precision, mfcc size): each must leave the staged-frame kernels
EDGES = ((257, (32, 16), 2, 40, "f32", 16),        # one frame beyond the longest window
         (257, (65, 32), 2, 40, "f32_fast", 16),
         (8, (145,), 145, 40, "f32", 16),          # layer 1 beyond 144: no matrix-core kernel at all, the per-layer kernel
         (8, (160,), 160, 40, "f32", 16),
         (8, (160, 16), 2, 40, "f32_fast", 16),
         (8, (32, 33), 2, 40, "f32", 16),          # a tail layer of 33
         (8, (65, 33), 2, 40, "f32_fast", 16),
         (8, (32, 16), 2, 31, "f32", 16),          # one window short of a tile
         (8, (65, 32), 2, 31, "f32_fast", 16),
         (8, (32, 16), 2, 40, "f32", 12),          # another mfcc size
         (8, (65, 32), 2, 40, "f32_fast", 12))


def case_id(case):
    return "L%d-%s-%d-w%d-%s" % (case[0], "x".join(map(str, case[1])) or "none", case[2], case[3], case[4]) + ("-K%d" % case[5] if len(case) > 5 else "")


# ------------------------------------------------------------------ models, streams, references
def _seed(*key):
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=None)
def model_of(dims):
    """N(0, 1 / in) weights, N(0, 0.01) biases, like tests/test_gpu_mlp_range_and_windows.py"""
    rng = np.random.default_rng(_seed("model", dims))
    ws = tuple(_frozen((rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(F32)) for i in range(len(dims) - 1))
    bs = tuple(_frozen((rng.standard_normal(dims[i + 1]) * 0.1).astype(F32)) for i in range(len(dims) - 1))
    return ws, bs


@functools.lru_cache(maxsize=None)
def streams(S, nf, k, key):
    """features on coefficient-dependent offsets ten times their spread, a level that drifts along the stream, a scale per stream"""
    rng = np.random.default_rng(_seed("mfcc", S, nf, k, key))
    off = rng.uniform(-30.0, 30.0, k).astype(F32)
    drift = np.linspace(0.0, 1.0, nf)[None, :, None] * rng.uniform(-6.0, 6.0, (S, 1, k))
    return _frozen((rng.standard_normal((S, nf, k)) * rng.uniform(0.5, 2.0, (S, 1, 1)) + off + drift).astype(F32))


def inputs_of(case):
    """(mfcc [S][n_win + L - 1][k], ws, bs) of a case"""
    k = case[5] if len(case) > 5 else K
    ws, bs = model_of(dims_of(case, k))
    return streams(streams_of(case), case[3] + case[0] - 1, k, case[:4]), ws, bs


def window_means(frames, L):
    """[n_win][k]: a window's column means as f32 sums in frame order (MfccNormalizer::normalize, window_means_body)"""
    n_win = frames.shape[0] - L + 1
    acc = np.zeros((n_win, frames.shape[1]), F32)
    for f in range(L):
        acc = acc + frames[f:f + n_win]
    return acc / F32(L)


def window_rows(frames, L):
    """[n_win][L * k] f32: every window minus its means, flattened -- what the model of the reference sees"""
    win = np.lib.stride_tricks.sliding_window_view(frames, L, axis=0).transpose(0, 2, 1)      # [n_win][L][k]
    return (win - window_means(frames, L)[:, None, :]).astype(F32).reshape(win.shape[0], -1)


def f64_forward(rows, ws, bs):
    h = np.asarray(rows, np.float64)
    for l, (w, b) in enumerate(zip(ws, bs)):
        h = h @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)
        if l + 1 < len(ws):
            h = np.maximum(h, 0.0)
    return h


def reference(mfcc, L, ws, bs):
    """[S][n_win][labels] f64: the normalised windows as the reference makes them (f32), the forward in float64"""
    return np.stack([f64_forward(window_rows(m, L), ws, bs) for m in mfcc])


def oracle(mfcc, L, ws, bs):
    """the same through the f32 oracle's forward (ModelImpl::forward): the second witness"""
    from oracle import rp_oracle as orc
    return np.stack([orc.mlp_forward(window_rows(m, L), list(ws), list(bs)) for m in mfcc])


@functools.lru_cache(maxsize=None)
def reference_of(case):
    mfcc, ws, bs = inputs_of(case)
    return _frozen(reference(mfcc, case[0], ws, bs))


def spread(mfcc, L):
    """the largest centred feature, sampled as test_window_logits_match_the_oracle samples it (every 16th window)"""
    S, nf = mfcc.shape[:2]
    return max(np.abs(mfcc[s, w:w + L] - mfcc[s, w:w + L].mean(axis=0)).max() for s in range(S) for w in range(0, nf - L + 1, 16))


def gate(ref, mfcc, L):
    """the project's logit gate: 1e-5 of the larger of the logit and the largest centred feature"""
    return 1e-5 * np.maximum(np.abs(ref), spread(mfcc, L))


# ------------------------------------------------------------------ the splits
def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _trunc(x, mask):
    return (_bits(x) & np.uint32(mask)).view(F32)


def split_bf16x3(x):
    """the kernels' three bf16 parts of a staged frame value, truncating and exact: x0 = x & 0xffff0000, r = x - x0, x1 = r & 0xffff0000,
    x2 = the upper half of r - x1 (mlp_windows_body, rp_mlp_windows.h:85-90)"""
    x = np.asarray(x, F32)
    x0 = _trunc(x, 0xffff0000)
    r = x - x0
    x1 = _trunc(r, 0xffff0000)
    return x0, x1, _trunc(r - x1, 0xffff0000)


def _bf16_rtn(x):
    u = _bits(x).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(F32)


def split_bf16x3_host(w):
    """bf16_split3 of the host (rp_ctx.cpp:316-333): rounded to nearest, truncated where the rounded parts do not add up to the weight"""
    w = np.asarray(w, F32)
    p0 = _bf16_rtn(w)
    r1 = w - p0
    p1 = _bf16_rtn(r1)
    p2 = _bf16_rtn(r1 - p1)
    bad = (p0 + p1) + p2 != w
    t0, t1, t2 = split_bf16x3(w)
    return np.where(bad, t0, p0), np.where(bad, t1, p1), np.where(bad, t2, p2)


def _rtz_f16(x):
    """v_cvt_pkrtz_f16_f32 of a value inside the f16 range, as f32: 11 significant bits, multiples of 2^-24 below 2^-14, towards zero"""
    x = np.asarray(x, F32)
    small = np.trunc(x.astype(np.float64) * 2.0 ** 24) / 2.0 ** 24
    return np.where(np.abs(x) >= 2.0 ** -14, _trunc(x, 0xffffe000), small.astype(F32))


def split_f16x2_frames(x):
    """the kernels' two f16 parts of a staged frame value: cvt_pkrtz(x), pk_f16_second(x - (x & 0xffffe000)) (rp_mlp_windows.h:92-94)"""
    x = np.asarray(x, F32)
    return _rtz_f16(x), _rtz_f16(x - _trunc(x, 0xffffe000))


def split_f16x2_weights(w):
    """the _Float16 pair of Model::create (rp_ctx.cpp:788): both rounded to nearest"""
    w = np.asarray(w, F32)
    w0 = w.astype(np.float16).astype(F32)
    return w0, (w - w0).astype(np.float16).astype(F32)


PRODUCTS = {"f32": tuple("x%dw%d" % (i, j) for i in range(3) for j in range(3) if i + j <= 2), "f32_fast": ("x0w0", "x1w0", "x0w1")}


def _splits(x, w, precision):
    if precision == "f32":
        return split_bf16x3(x), split_bf16x3_host(w)
    return split_f16x2_frames(x), split_f16x2_weights(w)


def emulate(mfcc, model, precision, drop=None, cap=MAX_TILES):
    """[S][n_win][labels] f64: what the staged-frame kernels compute, every sum in float64 -- per workgroup of the restated cut the frames
    minus the middle window's means c (f32), split, the product set of the form (PRODUCTS) less `drop`, the rest of a window's own mean
    taken out through the weight sums, bias, ReLU, the tail layers"""
    ws, bs = model
    L = ws[0].shape[1] // K
    dims = (ws[0].shape[1],) + tuple(w.shape[0] for w in ws)
    S, nf = mfcc.shape[:2]
    n_win = nf - L + 1
    _, nt, _, _, _ = route(dims, K, n_win, precision, cap=cap)
    assert nt > 0
    w1 = np.asarray(ws[0], F32)
    wsum = w1.reshape(-1, L, K).astype(np.float64).sum(axis=1).astype(F32).astype(np.float64)       # Model::wsum_for: f64 sums, kept as f32
    out = []
    for m in mfcc:
        mu = window_means(m, L)
        h1 = np.empty((n_win, w1.shape[0]))
        for w0, rows in workgroups(n_win, nt):
            c = mu[w0 + rows // 2]
            xs = (m[w0:w0 + rows + L - 1] - c).astype(F32)
            win = np.lib.stride_tricks.sliding_window_view(xs, L, axis=0).transpose(0, 2, 1).reshape(rows, -1)
            xp, wp = _splits(win, w1, precision)
            acc = np.zeros((rows, w1.shape[0]))
            for p in PRODUCTS[precision]:
                if p != drop:
                    acc += xp[int(p[1])].astype(np.float64) @ wp[int(p[3])].astype(np.float64).T
            h1[w0:w0 + rows] = acc - (mu[w0:w0 + rows] - c).astype(F32).astype(np.float64) @ wsum.T + np.asarray(bs[0], np.float64)
        if len(ws) > 1:
            h1 = f64_forward(np.maximum(h1, 0.0), ws[1:], bs[1:])
        out.append(h1)
    return np.stack(out)


# ------------------------------------------------------------------ every partial product is present
PARTS_L = 8
PARTS_MODELS = ((32, 96), (65, 97))      # (layer-1 width, windows): narrow NT 3, its pairing of tiles both taken and not; wide NT 4
PARTS_PATTERNS = {"ones": 0x7fffff, "parts": 0b11111110110111110111111}
PARTS_CASES = tuple((d1, n_win, prec, pat) for d1, n_win in PARTS_MODELS for prec in PRECISIONS for pat in PARTS_PATTERNS)
# the products of each form that CAN miss the gate by 8x when they go missing, on which weight pattern (module docstring)
PARTS_SHOW = {("f32", "ones"): ("x0w0", "x1w0"), ("f32", "parts"): ("x0w0", "x1w0", "x0w1"),
              ("f32_fast", "ones"): ("x0w0", "x1w0"), ("f32_fast", "parts"): ("x0w0", "x1w0", "x0w1")}


def _magnitudes(rng, shape, mantissa):
    """f32 values with the given 23 mantissa bits and exponents that put them in [0.5, 4)"""
    e = rng.integers(126, 129, size=shape).astype(np.uint32)
    return ((e << np.uint32(23)) | np.uint32(mantissa)).view(F32)


@functools.lru_cache(maxsize=None)
def parts_inputs(d1, n_win, pattern):
    """(mfcc [2][n_win + 7][16], (W,), (b,)): streams of +v, -v, +v ..; sign(W[o][f][k]) = (-1)^f sign(v[k]); no bias"""
    rng = np.random.default_rng(_seed("parts", d1, n_win, pattern))
    L, nf = PARTS_L, n_win + PARTS_L - 1
    sign = rng.choice(np.array([-1.0, 1.0], F32), size=K)
    v = _magnitudes(rng, (2, K), 0x7fffff) * sign
    alt = np.where(np.arange(nf) % 2 == 0, F32(1), F32(-1))
    mfcc = (alt[None, :, None] * v[:, None, :]).astype(F32)
    w = _magnitudes(rng, (d1, L, K), PARTS_PATTERNS[pattern]) * sign[None, None, :] * alt[None, :L, None]
    return _frozen(mfcc), (_frozen(w.reshape(d1, L * K).astype(F32)),), (_frozen(np.zeros(d1, F32)),)


def parts_magnitudes(mfcc, ws):
    """[S][n_win][d1] f64: sum|x||w| of every logit"""
    L = ws[0].shape[1] // K
    aw = np.abs(np.asarray(ws[0], np.float64)).T
    return np.stack([np.abs(np.lib.stride_tricks.sliding_window_view(m, L, axis=0).transpose(0, 2, 1).reshape(m.shape[0] - L + 1, -1)
                            .astype(np.float64)) @ aw for m in mfcc])


def parts_truncation(mfcc, ws, precision):
    """t: the largest share of sum|x||w| that the form leaves out by design on these inputs, from the splits themselves -- three parts: the
    products with i + j >= 3; two parts: x1 w1, what the second part of a frame value cuts (times |w|) and what the rounded second part
    of a weight misses (times |x0 + x1|).  The frames are staged as they are here (c = 0)."""
    L = ws[0].shape[1] // K
    w = np.asarray(ws[0], F32)
    worst = 0.0
    for m, mag in zip(mfcc, parts_magnitudes(mfcc, ws)):
        win = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(m, L, axis=0).transpose(0, 2, 1).reshape(mag.shape[0], -1))
        xp, wp = _splits(win, w, precision)
        xa = [np.abs(p.astype(np.float64)) for p in xp]
        wa = [np.abs(p.astype(np.float64)) for p in wp]
        if precision == "f32":
            left = xa[1] @ wa[2].T + xa[2] @ wa[1].T + xa[2] @ wa[2].T
        else:
            xr = np.abs(win.astype(np.float64) - xp[0] - xp[1])
            wr = np.abs(w.astype(np.float64) - wp[0] - wp[1])
            left = xa[1] @ wa[1].T + xr @ np.abs(w.astype(np.float64)).T + np.abs(xp[0].astype(np.float64) + xp[1]) @ wr.T
        worst = max(worst, float((left / mag).max()))
    return worst


def parts_gate(mfcc, ws, precision):
    """((16 L + 8) 2^-24 + t) sum|x||w| per logit"""
    L = ws[0].shape[1] // K
    return ((16 * L + 8) * 2.0 ** -24 + parts_truncation(mfcc, ws, precision)) * parts_magnitudes(mfcc, ws)


# ------------------------------------------------------------------ a large frame inside the middle window
HOT_L = 20
HOT_CASES = tuple((hidden, n_win, prec, value) for hidden in ((32, 16), (65, 32)) for n_win in (96, 225) for prec in PRECISIONS
                  for value in (1e4, 1e6))      # 225 windows: two workgroups per stream, so that one has a neighbour


def hot_frame(n_win, nt):
    """the frame in the middle of the middle window of the stream's first workgroup"""
    w0, rows = workgroups(n_win, nt)[0]
    return w0 + rows // 2 + HOT_L // 2
