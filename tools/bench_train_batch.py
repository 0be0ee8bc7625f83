"""Training of many personal wakeword models: ONE rp_wakeword_model_train_batch call against a loop of rp_wakeword_model_train over the same
sample sets, in one process.  W Tiny models, each trained on 5 synthetic wakeword recordings and 5 noise recordings (0.8-1.2 s, 16-bit PCM,
16 kHz) and tested on one of each, mfcc_size 16, for a FIXED number of epochs (--epochs, default 100; the reference's CLI trains for about
1 000) at learning rate 0.03.  Model w draws its weights from seed 1 + w in both forms.  The C arrays of both forms are built before the
clock starts; the two forms alternate, one warm-up round each, `--repeats` timed rounds; medians and spread in ms.  The results of both
forms are compared byte for byte once.  Of the batch call the tool also reports the feature stage (wav decoding and MFCCs, which the call
still runs one sample after the other: a batched MFCC front for training samples is not built) and the longest single kernel launch, both
from one extra call with the context's timing on, outside the timed rounds.

The yardstick is the loop of single calls.  No ratio is promised.  At W = 1 the batch call LOSES (measured: 7.76 ms against 6.48, 0.84x,
profiles/bench_train_batch.json): it runs ONE workgroup where the loop's kernels have the whole device per launch.  From there on it is
bound by the feature stage (0.8 of the call at W = 64 and 1 024).
One JSON line per W; all lines go to --out.
usage: python tools/bench_train_batch.py [--models 1,64,1024] [--epochs 100] [--repeats 5] [--out profiles/bench_train_batch.json]"""
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
from rustpotter_amd.api import _TrainOptions

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="1,64,1024")
ap.add_argument("--epochs", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join("profiles", "bench_train_batch.json"))
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs a GPU"
assert args.repeats >= 5, "medians over at least five rounds"

ctx = ra.BatchContext(0, host_pointers=True)
L = ra.load_library()
MFCC_SIZE, LR, N_WORD, N_NOISE = 16, 0.03, 5, 5
N_TRAIN, N_TEST = N_WORD + N_NOISE, 2


def wav_i16(x):
    data = np.clip(np.round(x * 32767), -32768, 32767).astype("<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, 1, 16000, 32000, 2, 16)
    return b"RIFF" + struct.pack("<I", 20 + len(fmt) + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + \
        struct.pack("<I", len(data)) + data


def recording(rng, word):
    n = int(rng.uniform(0.8, 1.2) * 16000)
    if not word:
        return wav_i16((0.05 * rng.standard_normal(n)).astype(np.float32))
    t = np.arange(n) / 16000.0
    f0 = rng.uniform(120, 400)
    x = sum(a * np.sin(2 * np.pi * f0 * h * t * (1 + 0.1 * np.sin(2 * np.pi * 3 * t))) for h, a in ((1, 0.3), (2, 0.15), (3, 0.08)))
    return wav_i16((x * np.sin(np.pi * t / t[-1]) ** 2 + 0.02 * rng.standard_normal(n)).astype(np.float32))


def c_set(names, wavs):
    n = len(names)
    return (C.c_char_p * n)(*names), (C.c_char_p * n)(*wavs), (C.c_size_t * n)(*[len(b) for b in wavs])


lines = []
for W in [int(x) for x in args.models.split(",")]:
    rng = np.random.default_rng(W)
    tr_names = [[b"w%d_%d[word %d].wav" % (w, i, w) for i in range(N_WORD)] + [b"n%d_%d.wav" % (w, i) for i in range(N_NOISE)] for w in range(W)]
    te_names = [[b"t%d[word %d].wav" % (w, w), b"tn%d.wav" % w] for w in range(W)]
    tr_wavs = [[recording(rng, i < N_WORD) for i in range(N_TRAIN)] for _ in range(W)]
    te_wavs = [[recording(rng, i == 0) for i in range(N_TEST)] for _ in range(W)]
    # the loop's arguments, one set per model
    one = [(c_set(tr_names[w], tr_wavs[w]), c_set(te_names[w], te_wavs[w])) for w in range(W)]
    # the batch call's
    b_tr = c_set([s for m in tr_names for s in m], [b for m in tr_wavs for b in m])
    b_te = c_set([s for m in te_names for s in m], [b for m in te_wavs for b in m])
    b_trc, b_tec = (C.c_size_t * W)(*([N_TRAIN] * W)), (C.c_size_t * W)(*([N_TEST] * W))
    seeds = (C.c_uint64 * W)(*[1 + w for w in range(W)])

    def loop(keep):
        res = []
        for w in range(W):
            opt = _TrainOptions(0, LR, args.epochs, 0, MFCC_SIZE, 1 + w)
            out, out_len = C.c_void_p(), C.c_size_t()
            (trn, trb, trl), (ten, teb, tel) = one[w]
            if L.rp_wakeword_model_train(ctx._h, C.byref(opt), N_TRAIN, trn, trb, trl, N_TEST, ten, teb, tel, None, 0, C.byref(out), C.byref(out_len),
                                         None, None) < 0:
                raise RuntimeError(L.rp_last_error().decode())
            if keep:
                res.append(C.string_at(out, out_len.value))
            L.rp_buffer_free(out)
        return res

    def batch(keep):
        opt = _TrainOptions(0, LR, args.epochs, 0, MFCC_SIZE, 1)
        outs, lens = (C.c_void_p * W)(), (C.c_size_t * W)()
        if L.rp_wakeword_model_train_batch(ctx._h, C.byref(opt), W, seeds, b_trc, *b_tr, b_tec, *b_te, None, None, outs, lens, None, None) < 0:
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
    ctx.timing_enable(True)
    batch(False)
    feature_ms, longest_ms, launches = ctx.train_batch_profile()
    ctx.timing_enable(False)
    res = {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in ms.items()}
    line = {"metric": "ms to train W Tiny wakeword models: one rp_wakeword_model_train_batch call against a loop of rp_wakeword_model_train",
            "models": W, "train_recordings_per_model": N_TRAIN, "test_recordings_per_model": N_TEST, "recording": "0.8-1.2 s, i16, 16 kHz",
            "mfcc_size": MFCC_SIZE, "epochs": args.epochs, "rounds": args.repeats, "ms": res,
            "loop_over_batch": round(res["loop"]["median_ms"] / res["batch"]["median_ms"], 2),
            "batch_feature_stage_ms": round(feature_ms, 3), "batch_feature_share": round(feature_ms / res["batch"]["median_ms"], 3),
            "batch_launches": launches, "batch_longest_launch_ms": round(longest_ms, 3),
            "bytes_equal": same, "device": torch.cuda.get_device_name(0), "build": ra.build_info()}
    print(json.dumps(line), flush=True)
    lines.append(json.dumps(line))
    with open(args.out, "w") as fh:   # after every W: a later, longer W that is cut short keeps the earlier lines
        fh.write("\n".join(lines) + "\n")
