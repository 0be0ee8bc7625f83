"""Host-only checks of the mixed-set entry points: they are declared in the header, exported, in the Python symbol list and in the Rust
binding (declaration and wrapper), and called with NULL handles they return -1 with an error text, without a device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rp_batch_detect_mixed_sets", "rp_frontend_batch_mixed_sets", "rp_stream_batch_new_mixed_sets", "rp_stream_batch_set_mixed_sets"]
WRAPPERS = {"rp_batch_detect_mixed_sets": "batch_detect_mixed_sets", "rp_frontend_batch_mixed_sets": "frontend_batch_mixed_sets",
            "rp_stream_batch_new_mixed_sets": "new_mixed_sets", "rp_stream_batch_set_mixed_sets": "set_mixed_sets"}


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
        assert re.search(r"pub fn %s\(" % name, rs), name                 # the declaration
        assert re.search(r"pub fn %s\(" % WRAPPERS[name], rs) and len(re.findall(r"\b%s\(" % name, rs)) >= 2, name   # and the wrapper that calls it
    # both rows and both banks, in the order of the header's contract
    sig = re.search(r"int\s+rp_batch_detect_mixed_sets\s*\(([^)]*)\)", hdr).group(1)
    order = ["rp_wakeword_bank *bank", "stream_wakewords", "ref_set_size", "rp_model_bank *model_bank", "stream_models", "model_set_size", "config",
             "precision", "*det,", "det_wakeword", "det_label", "n_det", "max_det"]
    at = [sig.index(w) for w in order]
    assert at == sorted(at), sig
    assert hasattr(rustpotter_amd.BatchContext, "batch_detect_mixed_sets") and hasattr(rustpotter_amd.BatchContext, "frontend_batch_mixed_sets")
    assert hasattr(rustpotter_amd.StreamBatch, "set_mixed_sets")


def test_null_handles_are_refused_without_a_device():
    import rustpotter_amd
    L = rustpotter_amd.load_library()
    assert L.rp_batch_detect_mixed_sets(None, None, 3, 0, 0, 0, None, None, 2, None, None, 2, None, 0, None, None, None, None, 0) == -1
    assert b"null handle" in L.rp_last_error()
    assert L.rp_frontend_batch_mixed_sets(None, None, 3, 0, 0, 0, None, None, None, 2, None, None, 2, None, 0, None, None) == -1
    assert b"null handle" in L.rp_last_error()
    assert L.rp_stream_batch_new_mixed_sets(None, None, None, 2, None, None, 2, None, 1, 1, None) == -1 and b"null handle" in L.rp_last_error()
    assert L.rp_stream_batch_set_mixed_sets(None, 0, 1, None, None) == -1 and b"null handle" in L.rp_last_error()


def test_the_constant_of_the_live_dtw_kernel():
    """RP_DTW_KERNEL_MIXED_SETS_STREAM = 65536 in the header, the Rust binding and the Python names of rp_ctx_dtw_kernels"""
    import rustpotter_amd
    hdr = re.sub(r"/\*.*?\*/", "", read("include", "rustpotter_hip.h"), flags=re.S)
    assert re.search(r"RP_DTW_KERNEL_MIXED_SETS_STREAM\s*=\s*65536\b", hdr)
    assert "pub const RP_DTW_KERNEL_MIXED_SETS_STREAM: c_int = 65536;" in read("bindings", "rustpotter_hip.rs")
    assert rustpotter_amd.BatchContext.DTW_KERNELS[65536] == "dtw_mixed_stream_kernel"


def test_the_kernels_are_new_sources_and_the_old_ones_are_where_they_were():
    """the resource tests list every kernel of these sources exactly.  Since the live-lane fold the mixed kernels sit beside their set twins
    (one targets kernel, one source for the set scans, the live DTW front next to dtw_set_stream_kernel); the two live forward fronts keep
    their own source, and the whole-recording and model-set sources hold nothing of mixed sets"""
    mk = read("rustpotter_amd", "csrc", "Makefile")
    for src, kernel in (("rp_gain_targets.hip", "stream_targets_kernel"), ("rp_scan_sets.hip", "scan_mixed_set_kernel"),
                        ("rp_scan_sets.hip", "scan_mixed_set_stream_kernel"), ("rp_dtw_set.hip", "dtw_mixed_stream_kernel"),
                        ("rp_mlp_mixed.hip", "window_means_mixed_stream_kernel"), ("rp_mlp_mixed.hip", "mlp_mixed_stream_kernel")):
        assert src in mk, src
        assert kernel in read("rustpotter_amd", "csrc", src)
    for gone in ("rp_mixed_targets.hip", "rp_scan_mixed.hip", "rp_dtw_mixed.hip", "rp_scan_set.hip", "rp_scan_model_set.hip"):
        assert gone not in mk and not os.path.exists(os.path.join(ROOT, "rustpotter_amd", "csrc", gone)), gone
    for src in ("rp_dtw_bank.hip", "rp_mlp_model_set.hip"):
        assert "mixed" not in read("rustpotter_amd", "csrc", src), src
