"""The inputs of the mixed-set tests (tests/mixed_set_cases.py) on the CPU: on the ORACLE's output they show what the feature is about --
references that win beside live models, models that win beside live references, both kinds winning in one stream, and a detector over both
rows that differs from the union of a reference-only and a model-only detector over the same audio (what two batches get wrong)."""
import mixed_set_cases as X
import model_set_cases as M


def test_bank_and_rows():
    assert X.REF_LENS == (42, 120, 207)
    lens = sorted({m[0] for m in M.MODELS})
    assert lens == [30, 47, 96, 195]
    assert lens[0] < X.REF_LENS[0] < lens[1] and lens[2] < X.REF_LENS[1] < lens[3] < X.REF_LENS[2]
    assert X.REF_ROWS.shape == X.MODEL_ROWS.shape == (X.S, 2) and X.S <= 12
    kinds = [(max(r) >= 0, max(m) >= 0) for r, m, _, _ in X.ROWS]
    assert (True, False) in kinds and (False, True) in kinds and (False, False) in kinds and kinds.count((True, True)) >= 5
    assert any(r[0] < 0 <= r[1] and m[0] < 0 <= m[1] for r, m, _, _ in X.ROWS), "a hole in front of a live slot on each side"
    assert any(r[0] == r[1] >= 0 and m[0] == m[1] >= 0 for r, m, _, _ in X.ROWS), "duplicates"
    assert X.pcm().shape == (X.S, 133 * 480)


def test_the_oracle_shows_the_feature():
    c = X.Cfg()
    x = X.pcm()
    none = (-1, -1)
    want = [X.oracle_detect(rr, mr, x[s], c) for s, (rr, mr, _, _) in enumerate(X.ROWS)]
    alone = [(X.oracle_detect(rr, none, x[s], c), X.oracle_detect(none, mr, x[s], c)) for s, (rr, mr, _, _) in enumerate(X.ROWS)]
    ref_wins, model_wins, both_kinds, differ = X.check_inputs(want, alone)
    print("references win %d detections beside live models, models %d beside live references; both kinds win in streams %s; streams %s "
          "differ from the union of two detectors" % (ref_wins, model_wins, both_kinds, differ))
    # a row without models is the reference-only detector, a row without references the model-only one
    for s, (rr, mr, _, _) in enumerate(X.ROWS):
        if max(mr) < 0:
            assert want[s] == alone[s][0]
        if max(rr) < 0:
            assert want[s] == alone[s][1]
