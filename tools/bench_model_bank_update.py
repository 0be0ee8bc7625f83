"""Adding n personal wakeword MODELS to a bank of W under a live-stream batch of 8 192 streams, in place against the only route there was
before a model bank could change.
  train:   (a) rp_model_bank_train into the bank the batch runs over, against (b) rp_wakeword_model_train_batch for the n, then
           rp_model_bank_new_from_rpw over all W + n files, then rp_stream_batch_new_model_bank.
  put_rpw: (a) rp_model_bank_put_from_rpw of n trained files, against (b) rp_model_bank_new_from_rpw over all W + n + a new batch.
What (a) buys first is not time: under (b) every connected stream loses its MFCC history and detector state.
A context with device pointers, the batch fed one chunk before the clock starts; Tiny models trained from 10 + 2 recordings (1 s, 16-bit
PCM, 16 kHz; five of the wakeword, five of noise; one of each to test on), 100 epochs; the bank's first W are 64 distinct models repeated;
the C arrays of both forms are built before the clock starts; the two forms alternate, one warm-up round each, `--repeats` timed rounds;
medians and spread in ms.  (a) always writes the slots W .. W + n - 1: from the second round on it replaces, and the bank's pools take the
garbage and grow as they do in service.  After the timed rounds one more (a) runs with rp_ctx_timing_enable: model_bank_put_kernel's own
time, by events around its launch (rp_model_bank_last_put_ms).  One JSON line per (form, W, n); all lines go to --out.
usage: python tools/bench_model_bank_update.py [--models 1024] [--add 1,64] [--streams 8192] [--repeats 5] [--out profiles/bench_model_bank_update.json]"""
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
ap.add_argument("--models", default="1024")
ap.add_argument("--add", default="1,64")
ap.add_argument("--streams", type=int, default=8192)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--epochs", type=int, default=100)
ap.add_argument("--out", default=os.path.join("profiles", "bench_model_bank_update.json"))
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs a GPU"
assert args.repeats >= 5, "medians over at least five rounds"

host = ra.BatchContext(0, host_pointers=True)    # trains the bank's first W models
ctx = ra.BatchContext(0, host_pointers=False)    # the measured context
L = ra.load_library()
DISTINCT, TRAIN, TEST, LR = 64, 10, 2, 0.027
S = args.streams


def check(r):
    if r < 0:
        raise RuntimeError(L.rp_last_error().decode())


def wav_i16(x):
    data = np.clip(np.round(x * 32767), -32768, 32767).astype("<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, 1, 16000, 32000, 2, 16)
    return b"RIFF" + struct.pack("<I", 20 + len(fmt) + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + \
        struct.pack("<I", len(data)) + data


def recording(rng, word):
    n = 16000
    t = np.arange(n) / 16000.0
    x = 0.05 * rng.standard_normal(n)
    if word:
        f0 = rng.uniform(120, 400)
        x = 0.4 * x + sum(a * np.sin(2 * np.pi * f0 * h * t * (1 + 0.1 * np.sin(2 * np.pi * 3 * t))) for h, a in ((1, 0.3), (2, 0.15), (3, 0.08))) * np.sin(np.pi * t / t[-1]) ** 2
    return wav_i16(x.astype(np.float32))


def sample_sets(rng, n, tag):
    """n models as BatchContext.train_wakeword_models takes them: (train, test), ordered {name: wav bytes}"""
    out = []
    for w in range(n):
        train = {"%s%d_n%d.wav" % (tag, w, i): recording(rng, False) for i in range(TRAIN // 2)}
        train.update({"%s%d_w%d[word].wav" % (tag, w, i): recording(rng, True) for i in range(TRAIN - TRAIN // 2)})
        test = {"%s%d_tn.wav" % (tag, w): recording(rng, False), "%s%d_tw[word].wav" % (tag, w): recording(rng, True)}
        assert len(test) == TEST
        out.append((train, test))
    return out


def pack(sets, n):
    names = [k.encode() for d in sets for k in d]
    bufs = [bytes(v) for d in sets for v in d.values()]
    m = len(names)
    return ((C.c_size_t * n)(*[len(d) for d in sets]), (C.c_char_p * m)(*names), (C.c_char_p * m)(*bufs), (C.c_size_t * m)(*[len(b) for b in bufs]))


rng = np.random.default_rng(1)
base = [g[0] for g in host.train_wakeword_models(sample_sets(rng, DISTINCT, "base"), m_type="tiny", learning_rate=LR, epochs=args.epochs)]
cfg = ra.DetectorConfig()
idx = torch.full((S,), -1, dtype=torch.int32, device="cuda")
chunk = torch.zeros((S, 480), dtype=torch.int16, device="cuda")
det = torch.zeros((S, 4, 24), dtype=torch.uint8, device="cuda")
n_det = torch.zeros((S,), dtype=torch.int32, device="cuda")
opt = _TrainOptions(0, LR, args.epochs, 0, 16, 1)


def live_batch(bank):
    sb = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=1, model_bank=bank, stream_model=idx.data_ptr())
    sb.process_dev(chunk.data_ptr(), 1, 1, 480, det.data_ptr(), n_det.data_ptr(), 4)
    return sb


lines = []
for W in [int(x) for x in args.models.split(",")]:
    first = [base[w % DISTINCT] for w in range(W)]
    for n in [int(x) for x in args.add.split(",")]:
        new = sample_sets(np.random.default_rng(1000 * W + n), n, "new")
        tr, te = pack([m[0] for m in new], n), pack([m[1] for m in new], n)
        new_files = [g[0] for g in host.train_wakeword_models(new, m_type="tiny", learning_rate=LR, epochs=args.epochs)]
        new_bufs = (C.c_char_p * n)(*new_files)
        new_lens = (C.c_size_t * n)(*[len(b) for b in new_files])
        all_bufs = (C.c_char_p * (W + n))(*(first + new_files))
        all_lens = (C.c_size_t * (W + n))(*[len(b) for b in first + new_files])
        loss, acc = (C.c_float * n)(), (C.c_float * n)()
        for form in ("train", "put_rpw"):
            # (a): the bank a service starts with, reserved, and the batch that stays
            bank = ra.ModelBank(ctx, rpw=first)
            bank.reserve(256, 4)
            sb = live_batch(bank)

            def in_place():
                if form == "train":
                    check(L.rp_model_bank_train(bank._h, W, n, C.byref(opt), None, *tr, *te, None, None, None, None, loss, acc))
                else:
                    check(L.rp_model_bank_put_from_rpw(bank._h, W, n, new_bufs, new_lens))

            def rebuild():
                if form == "train":
                    outs, out_lens = (C.c_void_p * n)(), (C.c_size_t * n)()
                    check(L.rp_wakeword_model_train_batch(ctx._h, C.byref(opt), n, None, *tr, *te, None, None, outs, out_lens, loss, acc))
                    for w in range(n):
                        all_bufs[W + w] = C.string_at(outs[w], out_lens[w])
                        all_lens[W + w] = out_lens[w]
                        L.rp_buffer_free(outs[w])
                h, b = C.c_void_p(), C.c_void_p()
                check(L.rp_model_bank_new_from_rpw(ctx._h, W + n, all_bufs, all_lens, C.byref(h)))
                check(L.rp_stream_batch_new_model_bank(ctx._h, h, idx.data_ptr(), C.byref(cfg._c()), S, 1, C.byref(b)))
                ctx.synchronize()
                L.rp_stream_batch_free(b)
                L.rp_model_bank_free(h)

            in_place()
            rebuild()   # the warm-up round of both forms
            ms = {"in_place": [], "rebuild": []}
            for _ in range(args.repeats):
                for k, fn in (("in_place", in_place), ("rebuild", rebuild)):
                    t0 = time.perf_counter()
                    fn()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            ctx.timing_enable(True)
            in_place()
            put_kernel_ms = bank.last_put_ms
            ctx.timing_enable(False)
            sb.process_dev(chunk.data_ptr(), 1, 1, 480, det.data_ptr(), n_det.data_ptr(), 4)   # the batch lives on over the changed bank
            ctx.synchronize()
            res = {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in ms.items()}
            calls = {"train": ("rp_model_bank_train", "rp_wakeword_model_train_batch + rp_model_bank_new_from_rpw over W + n + rp_stream_batch_new_model_bank"),
                     "put_rpw": ("rp_model_bank_put_from_rpw", "rp_model_bank_new_from_rpw over W + n + rp_stream_batch_new_model_bank")}[form]
            line = {"metric": "ms to add n models to a bank of W under a live batch: %s against %s (freeing the rebuilt bank and batch included)" % calls,
                    "form": form, "models": W, "added": n, "streams": S, "model": "Tiny, %d + %d recordings of 1 s (i16, 16 kHz), %d epochs" % (TRAIN, TEST, args.epochs),
                    "train_size": bank._L.rp_model_bank_train_size(bank._h, W), "rounds": args.repeats, "ms": res,
                    "rebuild_over_in_place": round(res["rebuild"]["median_ms"] / res["in_place"]["median_ms"], 2),
                    "model_bank_put_kernel_ms": round(put_kernel_ms, 4), "pool_growths": bank.pool_growths,
                    "bank_size_after": bank._L.rp_model_bank_size(bank._h), "device": torch.cuda.get_device_name(0), "build": ra.build_info()}
            print(json.dumps(line), flush=True)
            lines.append(json.dumps(line))
            with open(args.out, "w") as fh:   # after every line: a later, longer case that is cut short keeps the earlier ones
                fh.write("\n".join(lines) + "\n")
            sb.close()
            del bank
