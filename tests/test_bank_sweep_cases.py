"""The cases that tests/test_gpu_bank_sweeps.py runs, judged from the oracle alone (no GPU): none of them is threshold-sensitive, most of
their streams fire -- every case fires, and most holders do with the 70-stream case left out too --, and together they reach the decisions a
bank kernel can get wrong.  The conditions are sweep_parity.bank_suite_problems, per family."""
import pytest

import sweep_parity as sp


@pytest.mark.parametrize("family", sp.BANK_FAMILIES)
def test_bank_sweep_cases_are_decisive(family):
    seed, n, shapes = sp.BANK_SUITE[family]
    problems, facts = sp.bank_suite_problems(family, seed, n, shapes)
    print(family, facts)
    assert not problems, "the suite's cases of %s: %s (choose another seed or pin)" % (family, "; ".join(problems))
