"""The cases that tests/test_gpu_model_set_sweeps.py runs, judged from the oracle alone (no GPU): none of them is set aside (the oracle's
events stay put under thresholds scaled by 1 -+ 1e-4), and together they hold at least one detection won by slot 0, one won by a later
slot, one in a row whose models have different windows, and one stream with a set that never fires."""
import pytest

import model_set_cases as M
import model_set_sweep as W


@pytest.fixture(scope="module")
def facts():
    f = {"slot0": 0, "later": 0, "mixed_windows": 0, "silent_sets": 0, "detections": 0}
    for family in W.FAMILIES:
        seed, n = W.SUITE[family]
        for k in range(n):
            case = W.make_case(family, seed, k)
            for row, ev in zip(case["rows"], W.oracle_events(case)):
                live = [int(mi) for mi in row if mi >= 0]
                if live and not ev:
                    f["silent_sets"] += 1
                for e in ev:
                    winner = int(e[2][1:].split(":")[0])
                    assert winner in live
                    f["detections"] += 1
                    f["slot0"] += winner == live[0]
                    f["later"] += winner != live[0]
                    f["mixed_windows"] += len({M.MODELS[mi][0] for mi in live}) > 1
    print(f)
    return f


def test_the_cases_reach_the_decisions(facts):
    assert facts["slot0"] >= 1 and facts["later"] >= 1 and facts["mixed_windows"] >= 1 and facts["silent_sets"] >= 1, facts


@pytest.mark.parametrize("family", W.FAMILIES)
def test_no_case_is_set_aside(family):
    seed, n = W.SUITE[family]
    aside = [k for k in range(n) if W.set_aside(W.make_case(family, seed, k))]
    assert not aside, "model sets %s: the oracle itself moves under thresholds scaled by 1 -+ 1e-4 in cases %s (choose another seed)" % (family, aside)
