"""What the whole-recording calls over a bank and the two stream-batch constructors over a bank answer to arguments they refuse, to no
streams, to indices outside the bank and to an empty bank: the return value and the FULL error text, written out here and not built from
the library's output.  The table pins the C ABI's behaviour as it is, including three things that look like oversights: the reference-bank
detect calls check max_det only for an empty bank (a non-empty one runs into the allocation of max_det = -1 detections), the constructors
refuse S == 0 where the calls answer 0, and rp_batch_detect_bank_sets over no streams fails without an error text on a context that has
not staged a third output yet.

S = 3 recordings of 480 x 8 samples (21 frames).  Reference bank: mfcc_size 5, two wakewords with windows of 3 and 5 frames (19 and 17
windows).  Model bank: the two smallest Tiny models of test_gpu_model_bank.py (windows of 30 and 195 frames: no window in 21 frames).
Under host pointers an index outside [-1, W) is refused before anything is written; under device pointers the kernels take it as "none":
an all-zero row and no detection."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_model_bank import bank_weights

pytestmark = pytest.mark.gpu
S, N, NF, K, MAX_DET, PITCH = 3, 480 * 8, 21, 5, 2, 19
DET_BYTES = 24   # sizeof(rp_batch_detection)

SCORE, SCORE_SETS, DETECT, DETECT_SETS, DETECT_MODEL = ("rp_dtw_score_bank", "rp_dtw_score_bank_sets", "rp_batch_detect_bank",
                                                        "rp_batch_detect_bank_sets", "rp_batch_detect_model_bank")
NEW, NEW_SETS = "rp_stream_batch_new_bank", "rp_stream_batch_new_bank_sets"
CALLS = (SCORE, SCORE_SETS, DETECT, DETECT_SETS, DETECT_MODEL)
ALL = CALLS + (NEW, NEW_SETS)
SETS = (SCORE_SETS, DETECT_SETS, NEW_SETS)
DETECTS = (DETECT, DETECT_SETS, DETECT_MODEL)

# case -> {call: (return value, error text)}; host pointers
REFUSED = {
    "null_ctx": {c: (-1, "null handle") for c in ALL},
    "null_bank": {c: (-1, "null handle") for c in ALL},
    "other_ctx": {c: (-1, "the bank belongs to another context") for c in ALL},
    "null_idx": {c: (-1, "null argument") for c in ALL},
    "max_det_neg": {DETECT: (-1, "HIP error in hipMalloc: out of memory"), DETECT_SETS: (-1, "HIP error in hipMalloc: out of memory"),
                    DETECT_MODEL: (-1, "max_det must be >= 0")},
    "max_det_neg_empty": {c: (-1, "max_det must be >= 0") for c in DETECTS},
    "stride": {c: (-1, "pcm_stride smaller than n_samples") for c in DETECTS},
    "stride_empty": {c: (-1, "pcm_stride smaller than n_samples") for c in DETECTS},
    "fmt_empty": {c: (-1, "unknown sample format") for c in DETECTS},
    "pitch": {c: (-1, "win_pitch 18 is smaller than the largest window count of the call (19)") for c in (SCORE, SCORE_SETS, DETECT, DETECT_SETS)},
    # (rp_batch_detect_bank_sets over no streams: test_detect_bank_sets_over_no_streams)
    "no_streams": {SCORE: (0, None), SCORE_SETS: (0, None), DETECT: (0, None), DETECT_MODEL: (0, None),
                   NEW: (-1, "rp_stream_batch_new_bank: S and max_chunks_per_call must be >= 1"),
                   NEW_SETS: (-1, "rp_stream_batch_new_bank_sets: S and max_chunks_per_call must be >= 1")},
    "idx_W": {SCORE: (-1, "stream 1: wakeword index 2 is outside the bank (-1 .. 1)"),
              SCORE_SETS: (-1, "stream 1, slot 1: wakeword index 2 is outside the bank (-1 .. 1)"),
              DETECT: (-1, "stream 1: wakeword index 2 is outside the bank (-1 .. 1)"),
              DETECT_SETS: (-1, "stream 1, slot 1: wakeword index 2 is outside the bank (-1 .. 1)"),
              DETECT_MODEL: (-1, "stream 1: model index 2 is outside the bank (-1 .. 1)"),
              NEW: (-1, "stream 1: wakeword index 2 is outside the bank (-1 .. 1)"),
              NEW_SETS: (-1, "stream 1, slot 1: wakeword index 2 is outside the bank (-1 .. 1)")},
    "idx_m2": {SCORE: (-1, "stream 1: wakeword index -2 is outside the bank (-1 .. 1)"),
               SCORE_SETS: (-1, "stream 1, slot 1: wakeword index -2 is outside the bank (-1 .. 1)"),
               DETECT: (-1, "stream 1: wakeword index -2 is outside the bank (-1 .. 1)"),
               DETECT_SETS: (-1, "stream 1, slot 1: wakeword index -2 is outside the bank (-1 .. 1)"),
               DETECT_MODEL: (-1, "stream 1: model index -2 is outside the bank (-1 .. 1)"),
               NEW: (-1, "stream 1: wakeword index -2 is outside the bank (-1 .. 1)"),
               NEW_SETS: (-1, "stream 1, slot 1: wakeword index -2 is outside the bank (-1 .. 1)")},
}
# what a refusing case changes in the arguments of a call that would succeed
CHANGES = {
    "null_ctx": dict(ctx=None), "null_bank": dict(bank=None), "other_ctx": dict(bank="other"), "null_idx": dict(idx=None),
    "max_det_neg": dict(max_det=-1), "max_det_neg_empty": dict(bank="empty", max_det=-1), "stride": dict(stride=N - 1),
    "stride_empty": dict(bank="empty", stride=N - 1), "fmt_empty": dict(bank="empty", fmt=7), "pitch": dict(win_pitch=PITCH - 1),
    "no_streams": dict(n=0), "idx_W": dict(bad=2), "idx_m2": dict(bad=-2),
}
PARAMS = [(call, case) for case, per in REFUSED.items() for call in ALL if call in per]


class Env:
    """one context with its banks (reference, model, both also empty) and the inputs, in host or device memory"""

    def __init__(self, ra, host):
        self.ra, self.host, self.L = ra, host, ra.load_library()
        self.ctx = ra.BatchContext(device=0, host_pointers=host)
        rng = np.random.default_rng(21)
        feats = [rng.standard_normal((n, K)).astype(np.float32) for n in (3, 5)]
        self.bank = ra.WakewordBank(self.ctx, wakewords=[([f], None, None, None) for f in feats])
        self.empty = ra.WakewordBank(self.ctx, wakewords=[])
        self.models = [ra.Model(self.ctx, ws, bs) for ws, bs in bank_weights()[:2]]
        self.model_bank = ra.ModelBank(self.ctx, models=self.models, none_index=[0, 0])
        self.model_empty = ra.ModelBank(self.ctx, models=[])
        self.cfg = ra.DetectorConfig()._c()
        self.pcm = self.put((rng.standard_normal((S, N)) * 0.1).astype(np.float32))
        self.mfcc = self.put(rng.standard_normal((S, NF, K)).astype(np.float32))
        self.kept = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        if self.host:
            return a
        import torch
        return torch.from_numpy(a).cuda()

    @staticmethod
    def ptr(b):
        return None if b is None else b.ctypes.data if isinstance(b, np.ndarray) else b.data_ptr()

    @staticmethod
    def get(b):
        return b if isinstance(b, np.ndarray) else b.cpu().numpy()

    def out(self, n_bytes):
        """an output array of n_bytes, every byte 0xA5"""
        return self.put(np.full(max(n_bytes, 1), 0xA5, np.uint8))

    def indices(self, call, bank, bad):
        """the call's index array: streams 0 and 1 with a wakeword, stream 2 without (an empty bank: nobody has one); bad: the index of
        stream 1 (sets: its slot 1, and under device pointers both slots of stream 2) instead"""
        none = bank == "empty" and self.host
        if call in SETS:
            idx = np.array([[-1, -1]] * 3 if none else [[0, -1], [1, 0], [-1, -1]], np.int32)
            if bad is not None:
                idx[1, 1] = bad
                if not self.host:
                    idx[2] = bad
        else:
            idx = np.array([-1, -1, -1] if none else [0, 1, -1], np.int32)
            if bad is not None:
                idx[1] = bad
        return idx

    def run(self, call, other=None, ctx="own", bank="own", idx="own", bad=None, n=S, max_det=MAX_DET, stride=N, fmt=3, win_pitch=PITCH):
        """-> (return value, error text, the outputs by name as numpy arrays)"""
        L, model = self.L, call == DETECT_MODEL
        h_ctx = self.ctx._h if ctx == "own" else None
        of = other if bank == "other" else self
        b = None if bank is None else ((of.model_empty if model else of.empty) if bank == "empty" else (of.model_bank if model else of.bank))
        h_bank = None if b is None else b._h
        di = None if idx is None else self.put(self.indices(call, bank, bad))
        slots = 2 if call in SETS else 1
        o = {}
        if call in (SCORE, SCORE_SETS):
            o["agg"], o["avg"] = self.out(S * slots * PITCH * 4), self.out(S * slots * PITCH * 4)
            head = (h_ctx, self.ptr(self.mfcc), n, NF, h_bank, self.ptr(di)) + ((2,) if call == SCORE_SETS else ())
            r = getattr(L, call)(*head, 0.22, 5, 0, 1, self.ptr(o["avg"]), self.ptr(o["agg"]), win_pitch)
        elif call in DETECTS:
            o["det"], o["n_det"] = self.out(S * MAX_DET * DET_BYTES), self.out(S * 4)
            if call != DETECT:
                o["col"] = self.out(S * MAX_DET * 4)   # det_wakeword / det_label
            head = (h_ctx, self.ptr(self.pcm), fmt, n, N, stride, h_bank, self.ptr(di))
            if model:
                r = L.rp_batch_detect_model_bank(*head, C.byref(self.cfg), 0, self.ptr(o["det"]), self.ptr(o["col"]), self.ptr(o["n_det"]), max_det)
            else:
                o["agg"], o["avg"] = self.out(S * slots * PITCH * 4), self.out(S * slots * PITCH * 4)
                mid = (2, C.byref(self.cfg), self.ptr(o["det"]), self.ptr(o["col"])) if call == DETECT_SETS else (C.byref(self.cfg), self.ptr(o["det"]))
                r = getattr(L, call)(*head, *mid, self.ptr(o["n_det"]), max_det, self.ptr(o["agg"]), self.ptr(o["avg"]), win_pitch)
        else:
            h = C.c_void_p()
            mid = (2, C.byref(self.cfg)) if call == NEW_SETS else (C.byref(self.cfg),)
            r = getattr(L, call)(h_ctx, h_bank, self.ptr(di), *mid, n, 1, C.byref(h))
            assert (r == 0) == bool(h.value)
            if h.value:
                L.rp_stream_batch_free(h)
        err = L.rp_last_error().decode()
        assert L.rp_ctx_synchronize(self.ctx._h) == 0
        self.kept.append((di, o))
        return r, err, {k: self.get(v) for k, v in o.items()}


@pytest.fixture(scope="module")
def ra():
    import rustpotter_amd
    return rustpotter_amd


@pytest.fixture(scope="module")
def host(ra):
    return Env(ra, True)


@pytest.fixture(scope="module")
def other(ra):
    return Env(ra, True)


@pytest.fixture(scope="module")
def dev(ra):
    return Env(ra, False)


def untouched(outs):
    return all((a == 0xA5).all() for a in outs.values())


@pytest.mark.parametrize("call,case", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_refusal(host, other, call, case):
    want_r, want_err = REFUSED[case][call]
    r, err, outs = host.run(call, other=other, **CHANGES[case])
    print("%s %s -> %d %r" % (call, case, r, err))
    assert r == want_r
    if want_err is not None:
        assert err == want_err
    assert untouched(outs)   # a refusal (and a call over no streams) writes nothing


def test_detect_bank_sets_over_no_streams(ra):
    """S == 0 with a det_wakeword array under host pointers: -1 and NO error text of its own while the context's third output staging
    buffer has never been reserved (a reservation of 0 bytes hands back its null pointer, which the call reads as a failure); 0 once any
    call has reserved it"""
    env = Env(ra, True)
    assert env.run(DETECT, bank=None)[:2] == (-1, "null handle")
    r, err, outs = env.run(DETECT_SETS, n=0)
    print("%s no streams, fresh context -> %d %r" % (DETECT_SETS, r, err))
    assert (r, err) == (-1, "null handle") and untouched(outs)
    assert env.run(DETECT_SETS)[0] == 0
    r, err, outs = env.run(DETECT_SETS, n=0)
    print("%s no streams, after a call -> %d %r" % (DETECT_SETS, r, err))
    assert r == 0 and untouched(outs)


@pytest.mark.parametrize("call", ALL)
def test_device_indices_outside_the_bank_are_no_wakeword(dev, call):
    """device pointers: W and -2 are taken as they are -- stream 1 (sets: its slot 1, and stream 2) scores and reports nothing"""
    for bad in (2, -2):
        r, err, outs = dev.run(call, bad=bad)
        print("%s device index %d -> %d %r" % (call, bad, r, err))
        assert r == 0
        if call in (SCORE, DETECT):
            agg, avg = (outs[k].view(np.float32)[:S * PITCH].reshape(S, PITCH) for k in ("agg", "avg"))
            assert agg[0].any() and not agg[1].any() and not avg[1].any() and not agg[2].any()
        if call in (SCORE_SETS, DETECT_SETS):
            agg, avg = (outs[k].view(np.float32)[:S * 2 * PITCH].reshape(S, 2, PITCH) for k in ("agg", "avg"))
            assert agg[0, 0].any() and agg[1, 0].any() and not agg[1, 1].any() and not avg[1, 1].any() and not agg[2].any()
        if call in (DETECT, DETECT_SETS):
            n_det = outs["n_det"].view(np.int32)[:S]
            assert n_det[2] == 0 and (call == DETECT_SETS or n_det[1] == 0)
        if call == DETECT_MODEL:
            assert not outs["n_det"].view(np.int32)[:S].any()


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("call", CALLS)
def test_empty_bank_answers_zeros(host, dev, call, mode):
    """a Rustpotter without wakewords: det, n_det, agg, avg and det_wakeword / det_label come back all zero, whatever they held"""
    env = host if mode == "host" else dev
    r, err, outs = env.run(call, bank="empty")
    print("%s empty bank, %s pointers -> %d %r" % (call, mode, r, err))
    assert r == 0
    size = {"det": S * MAX_DET * DET_BYTES, "n_det": S * 4, "col": S * MAX_DET * 4, "agg": S * (2 if call in SETS else 1) * PITCH * 4}
    size["avg"] = size["agg"]
    for name, a in outs.items():
        assert not a[:size[name]].any(), name
