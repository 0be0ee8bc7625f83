"""Enrolment of many wakewords: ONE rp_wakeword_ref_build_batch call against a loop of rp_wakeword_ref_build over the same wakewords, in
one process.  W synthetic wakewords of 5 recordings each (0.8-1.2 s, 16-bit PCM, 16 kHz); the C arrays of both forms are built before the
clock starts; the two forms alternate, one warm-up round each, `--repeats` timed rounds; medians and spread in ms.  The results of both forms
are compared byte for byte once.  One JSON line per W; all lines go to --out.
usage: python tools/bench_enrol.py [--wakewords 64,1024,8192] [--repeats 5] [--mfcc-size 16] [--out profiles/bench_enrol_batch.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import rustpotter_amd as ra

ap = argparse.ArgumentParser()
ap.add_argument("--wakewords", default="64,1024,8192")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--mfcc-size", type=int, default=16)
ap.add_argument("--out", default=os.path.join("profiles", "bench_enrol_batch.json"))
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs a GPU"
assert args.repeats >= 5, "medians over at least five rounds"

ctx = ra.BatchContext(0, host_pointers=True)
L = ra.load_library()
RECORDINGS = 5


def wav_i16(x):
    data = np.clip(np.round(x * 32767), -32768, 32767).astype("<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, 1, 16000, 32000, 2, 16)
    return b"RIFF" + struct.pack("<I", 20 + len(fmt) + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + \
        struct.pack("<I", len(data)) + data


def recording(rng):
    n = int(rng.uniform(0.8, 1.2) * 16000)
    t = np.arange(n) / 16000.0
    f0 = rng.uniform(120, 400)
    x = sum(a * np.sin(2 * np.pi * f0 * h * t * (1 + 0.1 * np.sin(2 * np.pi * 3 * t))) for h, a in ((1, 0.3), (2, 0.15), (3, 0.08)))
    return wav_i16((x * np.sin(np.pi * t / t[-1]) ** 2 + 0.02 * rng.standard_normal(n)).astype(np.float32))


lines = []
for W in [int(x) for x in args.wakewords.split(",")]:
    rng = np.random.default_rng(W)
    names = [b"wakeword %d" % w for w in range(W)]
    snames = [[b"w%d_%d.wav" % (w, i) for i in range(RECORDINGS)] for w in range(W)]
    wavs = [[recording(rng) for _ in range(RECORDINGS)] for _ in range(W)]
    # the loop's arguments, one set per wakeword
    one = [((C.c_char_p * RECORDINGS)(*snames[w]), (C.c_char_p * RECORDINGS)(*wavs[w]), (C.c_size_t * RECORDINGS)(*[len(b) for b in wavs[w]]))
           for w in range(W)]
    # the batch call's
    n = W * RECORDINGS
    b_names = (C.c_char_p * W)(*names)
    b_counts = (C.c_size_t * W)(*([RECORDINGS] * W))
    b_snames = (C.c_char_p * n)(*[s for ww in snames for s in ww])
    b_wavs = (C.c_char_p * n)(*[b for ww in wavs for b in ww])
    b_lens = (C.c_size_t * n)(*[len(b) for ww in wavs for b in ww])

    def loop(keep):
        res = []
        for w in range(W):
            out, out_len = C.c_void_p(), C.c_size_t()
            if L.rp_wakeword_ref_build(ctx._h, names[w], None, None, RECORDINGS, one[w][0], one[w][1], one[w][2], args.mfcc_size, 1,
                                       C.byref(out), C.byref(out_len)) < 0:
                raise RuntimeError(L.rp_last_error().decode())
            if keep:
                res.append(C.string_at(out, out_len.value))
            L.rp_buffer_free(out)
        return res

    def batch(keep):
        outs, lens = (C.c_void_p * W)(), (C.c_size_t * W)()
        if L.rp_wakeword_ref_build_batch(ctx._h, W, b_names, None, None, b_counts, b_snames, b_wavs, b_lens, args.mfcc_size, 1, outs, lens) < 0:
            raise RuntimeError(L.rp_last_error().decode())
        res = [C.string_at(outs[w], lens[w]) for w in range(W)] if keep else []
        for w in range(W):
            L.rp_buffer_free(outs[w])
        return res

    same = loop(True) == batch(True)   # the warm-up round of both forms
    ms = {"loop": [], "batch": []}
    for _ in range(args.repeats):
        for k, fn in (("loop", loop), ("batch", batch)):
            t0 = time.perf_counter()
            fn(False)
            ms[k].append((time.perf_counter() - t0) * 1e3)
    res = {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in ms.items()}
    line = {"metric": "ms to enrol W wakewords: one rp_wakeword_ref_build_batch call against a loop of rp_wakeword_ref_build",
            "wakewords": W, "recordings_per_wakeword": RECORDINGS, "recording": "0.8-1.2 s, i16, 16 kHz", "mfcc_size": args.mfcc_size,
            "rounds": args.repeats, "ms": res, "loop_over_batch": round(res["loop"]["median_ms"] / res["batch"]["median_ms"], 2),
            "bytes_equal": same, "device": torch.cuda.get_device_name(0), "build": ra.build_info()}
    print(json.dumps(line), flush=True)
    lines.append(json.dumps(line))
    with open(args.out, "w") as fh:   # after every W: a later, longer W that is cut short keeps the earlier lines
        fh.write("\n".join(lines) + "\n")
