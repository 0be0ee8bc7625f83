"""Randomised parity sweeps for model sets against the oracle's chunked detector with one add_model per live slot (tests/model_set_sweep.py):
four whole-recording cases (rp_batch_detect_model_bank_sets) and four live cases (a batch over model sets fed in random pieces).  Events
exact -- chunk, counter, the winner's bank index and its label --, scores within 1e-4 with floor 1e-3.  No case is set aside:
tests/test_model_set_sweep_cases.py shows from the oracle alone that none of them hangs on a threshold."""
import pytest

import model_set_cases as M
import model_set_sweep as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


@pytest.fixture(scope="module")
def bank(ra, ctx):
    return ra.ModelBank(ctx, models=[ra.Model(ctx, ws, bs) for ws, bs in M.bank_weights()], none_index=M.NONE_INDEX)


@pytest.mark.parametrize("family,k", [(f, k) for f in W.FAMILIES for k in range(W.SUITE[f][1])])
def test_model_set_sweep(ra, ctx, bank, family, k):
    n = W.run_case(ra, ctx, bank, family, k)
    print("model sets %s case %d: %d detections, equal to the oracle's" % (family, k, n))
    assert n >= 1
