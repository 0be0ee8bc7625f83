"""The case list of tests/test_gpu_mlp_stream_edges.py proves its own coverage here, without a GPU: CASES reaches every class of walk that
Model::stream_plan's formula can produce, the integer models keep the premise that makes every arithmetic exact, the model rotation lets
each model meet each arithmetic and both `par` values, and the knob table reaches every build of mlp_stream_kernel that a knob can select."""
import itertools

import numpy as np

import mlp_stream_cases as M


def test_plan_restates_the_known_shapes():
    """the figures DESIGN.md 4.4 and rp_mlp_stream.hip quote: 3 120 floats = 97.5 lines, odd rows four chunks in; 64 floats at an aligned base
    is the one-unit tile"""
    p = M.plan(3120, 0)
    assert (p["par"], p["q1"], p["lines"], p["units"], p["flush"]) == (1, 4, 98, 49, True)
    p = M.plan(64, 0)
    assert (p["par"], p["q1"], p["lines"], p["units"], p["flush"]) == (0, 0, 2, 1, True)
    assert M.plan(64, 3)["units"] == 2 and not M.plan(64, 3)["flush"]       # three lines: the fourth k-step holds nothing
    assert not M.plan(96, 0)["flush"] and M.plan(96, 0)["lines"] == 3       # in % 64 == 32: the flush step is skipped at small phases
    # the lane groups that find a chunk in the next line: none at phase 0, the upper halves from phase 1, every one at phase 7 but lk 0's lower half
    assert M.plan(64, 0)["nx"][0] == ((False, False),) * 4
    assert M.plan(64, 1)["nx"][1] == ((False, False), (False, False), (False, False), (False, True))
    assert M.plan(64, 7)["nx"][7] == ((False, True), (True, True), (True, True), (True, True))
    assert sorted(M.plan(80, 2)["nx"]) == [2, 6]                            # par = 1: both phases in one launch


def test_cases_cover_every_class_of_walk():
    grid = list(itertools.product(M.INS, range(8)))
    assert set(M.CASES) <= set(grid) and len(set(M.CASES)) == len(M.CASES) <= 60
    want = {M.plan_class(n, q) for n, q in grid}
    got = {M.plan_class(n, q) for n, q in M.CASES}
    assert got == want and len(want) == 50
    # and the factors one by one, so that a change of plan_class cannot empty the statement above
    plans = [(n, q, M.plan(n, q)) for n, q in M.CASES]
    for par in (0, 1):
        assert {q for n, q, p in plans if p["par"] == par} == set(range(8))
        for flush in (False, True):
            assert any(p["par"] == par and p["flush"] == flush for _, _, p in plans)
        for odd in (0, 1):
            assert any(p["par"] == par and p["lines"] % 2 == odd for _, _, p in plans)
    for flush, odd in itertools.product((False, True), (0, 1)):
        have = {q for n, q, p in plans if p["flush"] == flush and p["lines"] % 2 == odd}
        assert have == {q for n, q in grid if M.plan(n, q)["flush"] == flush and M.plan(n, q)["lines"] % 2 == odd}, (flush, odd)
    assert any(p["units"] == 1 for _, _, p in plans) and any(p["units"] >= 3 for _, _, p in plans) and any(p["units"] >= 49 for _, _, p in plans)
    assert {n % 64 for n, _ in M.CASES} == {0, 16, 32, 48}
    assert {n for n, _ in M.CASES} == set(M.INS)
    # every true / false pattern of (nx0, nx1) over the four lane groups that a phase can make, at both parities of the line count
    for odd in (0, 1):
        assert {p["nx"][q] for _, _, p in plans if p["lines"] % 2 == odd for q in p["nx"]} == {M.plan(64, q)["nx"][q] for q in range(8)}


def test_model_rotation_meets_every_arithmetic_and_both_parities():
    met = {(mi, a, M.plan(n, 0)["par"]) for n in M.INS for a in range(len(M.ARITH)) for mi in M.models_for(n, a)}
    assert {(mi, a) for mi, a, _ in met} == set(itertools.product(range(len(M.MODELS)), range(len(M.ARITH))))
    assert {(mi, par) for mi, _, par in met} == set(itertools.product(range(len(M.MODELS)), (0, 1)))
    assert {n for n, _ in M.CASES} == set(M.INS)   # and CASES walks every one of those row lengths
    # the multi-tile rotation (shift 5) brings the two-round tail layers and the f16 pair's redo list to both row lengths' tile boundaries
    assert {M.MODELS[mi] for n in (64, 80) for a in range(4) for mi in M.models_for(n, a, 5)} >= {(16, (100, 5)), (17, (37, 3)), (1, (1,)), (16, ())}


def test_models_are_the_issue_s_list():
    assert set(M.MODELS) >= {(1, ()), (16, ()), (17, ()), (32, ()), (13, (2,)), (32, (16, 2)), (17, (37, 3)), (32, (100, 5)), (1, (1,))}
    # the tail loop's second round of 32 inputs needs a model that mlp_stream_kernel has room for: (32, (100, 5)) is not one (its route is
    # asserted on the GPU), (17, (37, 3)) and the twin (16, (100, 5)) are
    for prec in M.ARITH:
        for n in M.INS:
            ok = {m: M.stream_supported(M.dims_of(n, m), prec) for m in M.MODELS}
            assert [m for m in ok if not ok[m]] == [(32, (100, 5))]
    assert M.MODELS[M.TWIN[M.MODELS.index((32, (100, 5)))]] == (16, (100, 5))


def _integer_model_checks(n, mi, B, seed=0):
    ws, bs = M.integer_model(n, mi)
    x = M.integer_rows(n, B, seed)
    dims = M.dims_of(n, M.MODELS[mi])
    assert x.shape == (B, n) and [w.shape for w in ws] == [(dims[i + 1], dims[i]) for i in range(len(dims) - 1)]
    assert np.array_equal(x, np.rint(x)) and np.abs(x).max() == 8
    assert all(np.array_equal(w, np.rint(w)) for w in ws + bs) and np.abs(ws[0]).max() <= 2
    layers = M.f64_layers(x, ws, bs)
    for l, (pre, bound) in enumerate(layers):
        assert bound.max() < 2 ** 24, (n, mi, l, bound.max())
        assert np.array_equal(pre, np.rint(pre))
        if l + 1 < len(layers):   # a hidden layer: the ReLU both passes and clips
            assert (pre > 0).any() and (pre < 0).any(), (n, mi, l)
    logits = M.integer_logits(n, mi, B, seed)
    assert logits.dtype == np.float32 and logits.shape == (B, dims[-1]) and np.array_equal(logits.astype(np.float64), layers[-1][0])
    assert len(np.unique(logits)) > 4 or B < 8   # not a constant


def test_integer_models_keep_every_partial_sum_below_2_24():
    """the premise of the exact tests, from the f64 evaluation, for every (row length, model) pair the GPU tests use"""
    for n in M.INS:
        for a in range(len(M.ARITH)):
            for mi in M.models_for(n, a):
                _integer_model_checks(n, mi, M.B_CASES)
    for n in (96, 80):                 # batch edges
        for a in range(len(M.ARITH)):
            for mi in M.models_for(n, a):
                _integer_model_checks(n, mi, 257, seed=1)
    for n in M.BUILD_INS:              # builds
        for mi in M.BUILD_MODELS:
            _integer_model_checks(n, mi, M.B_CASES)


def test_multi_tile_batches_and_samples():
    for n_cu in (64, 256, 304):
        for n, waves in ((64, 8), (64, 4), (80, 8)):
            par = M.plan(n, 0)["par"]
            B = M.multi_tile_B(n, n_cu, waves)
            assert B * n * 4 < 48 << 20
            nbt, grid = M.n_tiles(B, par, waves), n_cu * (8 // waves)
            assert 2 * grid < nbt < (5 if waves == 4 else 3) * grid    # some workgroups walk one tile more than others
            assert B % (16 * waves) not in (0, 16 * waves - 1)       # a ragged last tile
            rows = M.multi_tile_sample(B, par, n_cu, waves)
            assert len(rows) == 512 == len(set(rows.tolist())) and rows.max() == B - 1
            tiles = {M.row_tile(int(r), par, waves) for r in rows}
            assert {bt // grid for bt in tiles if bt % grid == 0} >= {0, 1, 2}   # workgroup 0's first, second and third tile
            assert {bt // grid for bt in tiles} >= {0, 1, 2} and nbt - 1 in tiles
    # the batch depends on the device's CU count: the models of these tests keep the exactness premise for ANY rows of features in [-8, 8]
    for n, waves in ((64, 8), (64, 4), (80, 8)):
        for a in range(len(M.ARITH)):
            for mi in M.models_for(n, a, 0 if waves == 4 else 5):
                assert M.integer_model_worst_case(n, mi) < 2 ** 24, (n, M.MODELS[mi])
                _integer_model_checks(n, mi, M.multi_tile_B(n, 16, waves), seed=2)


def test_knob_table_reaches_every_build_a_knob_can_select():
    """launch_mlp_stream's choice restated: over the builds test's models, arithmetics and knobs every (NT, PREC, D, waves) instantiation that
    a knob can select is run -- all but <2, bf16x3, 2, 8>, whose weight ring never fits beside eight waves' row rings"""
    reached = set()
    for n in M.BUILD_INS:
        for mi in M.BUILD_MODELS:
            dims = M.dims_of(n, M.MODELS[mi])
            for prec in M.ARITH:
                for knob in M.KNOBS:
                    depth, waves, moved = M.stream_build(dims, prec, knob)
                    reached.add(((dims[1] + 15) // 16, prec, depth, waves))
                    rep = M.stream_report(dims, prec, knob)
                    assert rep.startswith("mlp_stream_kernel<") and ("[stream build" in rep) == moved
                    if not knob:
                        assert not moved
    want = {(nt, prec) + ring for nt in (1, 2) for prec in M.ARITH for ring in ((2, 8), (1, 8), (1, 4))}
    want |= {(nt, "f32", 2, 6) for nt in (1, 2)}
    want.discard((2, "f32", 2, 8))
    assert reached == want
    # the refusals the GPU test meets: two four-wave workgroups of a two-tile model with tail layers do not fit a CU in the three-part form
    assert M.stream_build((96, 32, 16, 2), "f32", {"RP_MLP_STREAM_WAVES": "4"}) == (1, 8, False)
    assert M.stream_build((96, 32), "f32", {"RP_MLP_STREAM_WAVES": "4"}) == (1, 4, True)
    assert M.stream_build((96, 32, 16, 2), "f32", {"RP_MLP_STREAM_DEPTH": "1"}) == (1, 8, False)    # the default there already
    assert M.stream_build((96, 32, 16, 2), "bf16", {"RP_MLP_STREAM_WAVES": "6"}) == (2, 8, False)   # the six-wave build is the three-part form's
    assert M.stream_build((96, 13, 2), "f32", {"RP_MLP_STREAM_WAVES": "6"}) == (2, 6, True)
