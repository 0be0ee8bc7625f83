"""Adding n wakewords to a bank of W under a live-stream batch of 8 192 streams: (a) rp_wakeword_bank_enrol into the bank the batch runs
over, against (b) the only route there was before a bank could change -- rp_wakeword_ref_build_batch for the n, rp_wakeword_bank_new_from_rpw
over all W + n, rp_stream_batch_new_bank.  What (a) buys first is not time: under (b) every connected stream loses its state.
A context with device pointers, the batch detect-only and fed one chunk before the clock starts; wakewords of 5 recordings each (0.8-1.2 s,
16-bit PCM, 16 kHz), the bank's first W are 64 distinct ones repeated; the C arrays of both forms are built before the clock starts; the two
forms alternate, one warm-up round each, `--repeats` timed rounds; medians and spread in ms.  (a) always writes the slots W .. W + n - 1: from
the second round on it replaces, and the bank's pools take the garbage and grow as they do in service.  One JSON line per (W, n); all lines
go to --out.
usage: python tools/bench_bank_update.py [--wakewords 1024,8192] [--add 1,64] [--streams 8192] [--repeats 5] [--out profiles/bench_bank_update.json]"""
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
ap.add_argument("--wakewords", default="1024,8192")
ap.add_argument("--add", default="1,64")
ap.add_argument("--streams", type=int, default=8192)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--mfcc-size", type=int, default=16)
ap.add_argument("--out", default=os.path.join("profiles", "bench_bank_update.json"))
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs a GPU"
assert args.repeats >= 5, "medians over at least five rounds"

host = ra.BatchContext(0, host_pointers=True)    # builds the bank's first W references
ctx = ra.BatchContext(0, host_pointers=False)    # the measured context
L = ra.load_library()
RECORDINGS, DISTINCT, MAX_LEN = 5, 64, 130
S, K = args.streams, args.mfcc_size


def check(r):
    if r < 0:
        raise RuntimeError(L.rp_last_error().decode())


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


def wakewords(rng, n, tag):
    return [("%s %d" % (tag, w), {"%s%d_%d.wav" % (tag, w, i): recording(rng) for i in range(RECORDINGS)}, None, None) for w in range(n)]


rng = np.random.default_rng(1)
base = host.build_wakeword_refs(wakewords(rng, DISTINCT, "base"), K)
cfg = ra.DetectorConfig()
idx = torch.full((S,), -1, dtype=torch.int32, device="cuda")
chunk = torch.zeros((S, 480), dtype=torch.int16, device="cuda")
det = torch.zeros((S, 4, 24), dtype=torch.uint8, device="cuda")
n_det = torch.zeros((S,), dtype=torch.int32, device="cuda")


def live_batch(bank):
    sb = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=1, bank=bank, stream_wakeword=idx.data_ptr())
    sb.process_dev(chunk.data_ptr(), 1, 1, 480, det.data_ptr(), n_det.data_ptr(), 4)
    return sb


lines = []
for W in [int(x) for x in args.wakewords.split(",")]:
    first = [base[w % DISTINCT] for w in range(W)]
    for n in [int(x) for x in args.add.split(",")]:
        new = wakewords(np.random.default_rng(1000 * W + n), n, "new")
        m = n * RECORDINGS
        names = (C.c_char_p * n)(*[w[0].encode() for w in new])
        counts = (C.c_size_t * n)(*([RECORDINGS] * n))
        snames = (C.c_char_p * m)(*[k.encode() for w in new for k in w[1]])
        wavs = (C.c_char_p * m)(*[b for w in new for b in w[1].values()])
        lens = (C.c_size_t * m)(*[len(b) for w in new for b in w[1].values()])
        all_bufs = (C.c_char_p * (W + n))(*first)
        all_lens = (C.c_size_t * (W + n))(*[len(b) for b in first])
        # (a): the bank a service starts with, reserved, and the batch that stays
        bank = ra.WakewordBank(ctx, rpw=first)
        bank.reserve(max_len=MAX_LEN)
        sb = live_batch(bank)

        def enrol():
            check(L.rp_wakeword_bank_enrol(bank._h, W, n, names, None, None, counts, snames, wavs, lens, 1, None, None))

        def rebuild():
            outs, out_lens = (C.c_void_p * n)(), (C.c_size_t * n)()
            check(L.rp_wakeword_ref_build_batch(ctx._h, n, names, None, None, counts, snames, wavs, lens, K, 1, outs, out_lens))
            for w in range(n):
                all_bufs[W + w] = C.string_at(outs[w], out_lens[w])
                all_lens[W + w] = out_lens[w]
                L.rp_buffer_free(outs[w])
            h, b = C.c_void_p(), C.c_void_p()
            check(L.rp_wakeword_bank_new_from_rpw(ctx._h, W + n, all_bufs, all_lens, C.byref(h)))
            check(L.rp_stream_batch_new_bank(ctx._h, h, idx.data_ptr(), C.byref(cfg._c()), S, 1, C.byref(b)))
            ctx.synchronize()
            L.rp_stream_batch_free(b)
            L.rp_wakeword_bank_free(h)

        enrol()
        rebuild()   # the warm-up round of both forms
        ms = {"enrol": [], "rebuild": []}
        for _ in range(args.repeats):
            for k, fn in (("enrol", enrol), ("rebuild", rebuild)):
                t0 = time.perf_counter()
                fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        sb.process_dev(chunk.data_ptr(), 1, 1, 480, det.data_ptr(), n_det.data_ptr(), 4)   # the batch lives on over the changed bank
        ctx.synchronize()
        res = {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in ms.items()}
        line = {"metric": "ms to add n wakewords to a bank of W under a live batch: rp_wakeword_bank_enrol against rp_wakeword_ref_build_batch + "
                          "rp_wakeword_bank_new_from_rpw over W + n + rp_stream_batch_new_bank (freeing the rebuilt bank and batch included)",
                "wakewords": W, "added": n, "streams": S, "recordings_per_wakeword": RECORDINGS, "recording": "0.8-1.2 s, i16, 16 kHz",
                "mfcc_size": K, "rounds": args.repeats, "ms": res,
                "rebuild_over_enrol": round(res["rebuild"]["median_ms"] / res["enrol"]["median_ms"], 2), "pool_growths": bank.pool_growths,
                "bank_size_after": bank._L.rp_wakeword_bank_size(bank._h), "device": torch.cuda.get_device_name(0), "build": ra.build_info()}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        with open(args.out, "w") as fh:   # after every line: a later, longer case that is cut short keeps the earlier ones
            fh.write("\n".join(lines) + "\n")
        sb.close()
        del bank
