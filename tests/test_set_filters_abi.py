"""Host-only checks of the gain normaliser on wakeword sets, model banks and model sets: the five new functions are exported, declared in the
header, the Python symbol list and the Rust binding; NULL handles are refused without a device; the preparation kernel is part of the build;
the calls that refused the gain normaliser before still refuse it with the texts they had, and the new call's own refusal names itself and
points to rp_stream_batch_set_filters."""
import math
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rp_model_bank_set_rms_levels", "rp_model_bank_rms_level", "rp_frontend_batch_bank_sets", "rp_frontend_batch_model_bank",
       "rp_stream_batch_set_filters_per_stream"]


def read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_the_new_functions_are_exported_and_declared():
    import rustpotter_amd
    from rustpotter_amd.api import SYMBOLS
    L = rustpotter_amd.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", read("include", "rustpotter_hip.h"), flags=re.S)
    rs = read("bindings", "rustpotter_hip.rs")
    for name in NEW:
        assert hasattr(L, name), name
        assert name in SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    # the levels mirror the two wakeword-bank functions word for word
    sig = lambda n: re.search(r"(\w+)\s+%s\s*\(([^)]*)\)" % n, hdr).groups()
    swap = lambda s: s.replace("rp_wakeword_bank", "rp_model_bank").replace("wakeword", "model")
    assert tuple(swap(x) for x in sig("rp_wakeword_bank_set_rms_levels")) == sig("rp_model_bank_set_rms_levels")
    assert tuple(swap(x) for x in sig("rp_wakeword_bank_rms_level")) == sig("rp_model_bank_rms_level")


def test_null_handles_are_refused_without_a_device():
    import rustpotter_amd
    L = rustpotter_amd.load_library()
    assert math.isnan(L.rp_model_bank_rms_level(None, 0)) and math.isnan(L.rp_model_bank_rms_level(None, -1))
    assert L.rp_model_bank_set_rms_levels(None, None) == -1 and b"null handle" in L.rp_last_error()
    assert L.rp_stream_batch_set_filters_per_stream(None, None) == -1 and b"null handle" in L.rp_last_error()
    for fn in (L.rp_frontend_batch_bank_sets, L.rp_frontend_batch_model_bank):
        assert fn(None, None, 3, 0, 0, 0, None, None, None, 1, None, 0, None, None) == -1 and b"null handle" in L.rp_last_error()


def test_the_preparation_kernel_is_built_and_the_gain_kernels_are_where_they_were():
    mk = read("rustpotter_amd", "csrc", "Makefile")
    assert "rp_gain_targets.hip" in mk
    src = read("rustpotter_amd", "csrc", "rp_gain_targets.hip")
    assert "stream_targets_kernel" in src and "__launch_bounds__(64)" in src
    fe = read("rustpotter_amd", "csrc", "rp_frontend.hip")
    for name in ("gain_per_stream_kernel", "lane_gain", "stream_filters_kernel"):
        assert name in fe and name not in src, name   # the existing per-stream kernels stay in rp_frontend.hip; the new file has none of them


def test_old_refusals_keep_their_texts_and_the_new_one_names_itself():
    sb = read("rustpotter_amd", "csrc", "rp_stream_batch.cpp")
    for text in ("the gain normaliser is not available on a batch over wakeword sets",
                 "the gain normaliser per model is not built for a batch over a model bank",
                 "rp_stream_batch_set_filters: the gain normaliser is not available on a batch over a model bank",
                 "rp_stream_batch_set_filters: the gain normaliser is not available on a batch over a wakeword bank",
                 "the batch was not made by rp_stream_batch_new_bank"):
        assert text in sb, text
    assert '"rp_stream_batch_set_filters_per_stream"' in sb
    assert re.search(r"the batch holds shared wakewords[^\"]*rp_stream_batch_set_filters takes them", sb)
