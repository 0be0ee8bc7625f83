"""The bank family through the randomised sweeps of tests/sweep_parity.py: wakeword banks, wakeword sets, a model bank and live batches over
them (resets, re-targets, set_models, puts that grow the pools under a running batch -- under a sets batch too --, per-stream filters,
resampled input) against the oracle's chunked single-stream detector, one orc.Detector per stream.  The whole-recording calls also run on
a context without host pointers, where an index outside the bank reaches the kernels and means "no wakeword".  Six cases per sweep (models:
four), the last with 70 streams; which cases these are, that the oracle sets none of them aside and that they reach the decisions is
asserted without a GPU in tests/test_bank_sweep_cases.py.  Long runs: profiles/sweep_banks.txt."""
import pytest

import sweep_parity as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def ctx(ra):
    return ra.BatchContext(device=0, host_pointers=True)


def run(ra, ctx, family, sweep):
    seed, n, shapes = sp.BANK_SUITE[family]
    cases, total, aside, secs = sweep(ra, ctx, n, seed, shapes=shapes)
    print("%s: %d cases, %d detections equal to the oracle's, %d set aside, %.1f s" % (family, cases, total, aside, secs))
    assert cases == n and aside == 0 and total > 0


def test_bank_sweep(ra, ctx):
    """rp_batch_detect_bank and rp_dtw_score_bank over whole recordings"""
    run(ra, ctx, "bank", sp.run_bank_sweep)


def test_bank_sets_sweep(ra, ctx):
    """rp_batch_detect_bank_sets: the reported wakeword is the bank index of the oracle's winner"""
    run(ra, ctx, "bank_sets", sp.run_bank_sets_sweep)


def test_live_bank_sweep(ra, ctx):
    """live batches over a bank with mid-run events"""
    run(ra, ctx, "live_bank", sp.run_live_bank_sweep)


def test_live_bank_sets_sweep(ra, ctx):
    """live batches over wakeword sets, with the slots' scores"""
    run(ra, ctx, "live_bank_sets", sp.run_live_bank_sets_sweep)


def test_model_bank_sweep(ra, ctx):
    """rp_batch_detect_model_bank and a live batch over the model bank with set_models events against orc.Detector.add_model"""
    run(ra, ctx, "model_bank", sp.run_model_bank_sweep)
