"""Filters for live-stream batches (rp_stream_batch_set_filters / rp_stream_batch_levels), the part that needs no GPU: the header
declares both functions, the library exports them, the Python harness lists them and takes the new arguments, and a NULL batch
is refused."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rp_stream_batch_set_filters", "rp_stream_batch_levels")


def test_header_declares_the_two_functions():
    src = open(os.path.join(ROOT, "include", "rustpotter_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+rp_stream_batch_set_filters\s*\(\s*rp_stream_batch\s*\*\s*b\s*,\s*const\s+rp_filters_config\s*\*\s*filters\s*,"
                     r"\s*float\s+rms_level_ref\s*\)\s*;", src)
    assert re.search(r"int\s+rp_stream_batch_levels\s*\(\s*rp_stream_batch\s*\*\s*b\s*,\s*float\s*\*\s*rms\s*,\s*float\s*\*\s*gains\s*\)\s*;", src)


def test_library_exports_them_and_refuses_a_null_batch():
    import ctypes as C
    import rustpotter_amd
    from rustpotter_amd.api import SYMBOLS, _FiltersCfg
    L = rustpotter_amd.load_library()
    for name in NEW:
        assert name in SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    f = _FiltersCfg()
    assert L.rp_stream_batch_set_filters(None, C.byref(f), 0.05) == -1 and L.rp_last_error()
    assert L.rp_stream_batch_levels(None, None, None) == -1 and L.rp_last_error()


def test_stream_batch_takes_filters():
    import rustpotter_amd
    p = inspect.signature(rustpotter_amd.StreamBatch.__init__).parameters
    assert "filters" in p and p["filters"].default is None
    assert "rms_level_ref" in p and p["rms_level_ref"].default != p["rms_level_ref"].default   # NaN: no reference level
    assert callable(getattr(rustpotter_amd.StreamBatch, "levels")) and callable(getattr(rustpotter_amd.StreamBatch, "set_filters"))


def test_rust_binding_declares_and_uses_them():
    rs = open(os.path.join(ROOT, "bindings", "rustpotter_hip.rs")).read()
    for name in NEW:
        assert len(re.findall(r"\b%s\s*\(" % name, rs)) >= 2, name   # the extern declaration and a wrapper that calls it
