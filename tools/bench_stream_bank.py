"""Personal wakewords on live streams: a live-stream batch over a wakeword bank (rp_stream_batch_new_bank: stream s holds wakeword s mod W)
against the shared-wakeword live batch (rp_stream_batch_new under RP_ARITH_STRICT_F32) with ONE wakeword of the same shape, in one process.
S streams fed `chunks` 30 ms chunks of synthetic i16 PCM per call from the device, mfcc_size 5, band 5, detect-only; W wakewords of 5 templates
of 90-110 frames with an averaged template.  Every (S, chunks, W) runs in a fresh process under its own time limit; the two batches alternate,
two warm-up rounds each, `--repeats` timed rounds of `--calls` process calls, medians in ms per call; the DTW launches of a call alone (kernel 1 of
rp_ctx_timing_read) for both.  bank_over_shared is the price of per-lane templates.  One JSON line per case; all lines go to --out.
usage: python tools/bench_stream_bank.py [--streams 8192,65536] [--chunks 1,8] [--wakewords 64,8192] [--repeats 5] [--out profiles/bench_stream_bank.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--streams", default="8192,65536")
ap.add_argument("--chunks", default="1,8")
ap.add_argument("--wakewords", default="64,8192")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=20, help="process calls per timed round")
ap.add_argument("--step-timeout", type=int, default=240)
ap.add_argument("--out", default=os.path.join("profiles", "bench_stream_bank.json"))
ap.add_argument("--child", default="", help="(internal) S,chunks,W: measure this case and print its line")
args = ap.parse_args()
assert args.repeats >= 5, "medians over at least five rounds"

if not args.child:
    lines = []
    for S in [int(x) for x in args.streams.split(",")]:
        for chunks in [int(x) for x in args.chunks.split(",")]:
            for W in [int(x) for x in args.wakewords.split(",")]:
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "%d,%d,%d" % (S, chunks, W),
                       "--repeats", str(args.repeats), "--calls", str(args.calls)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:   # nothing more is started on the device after a step that failed
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    sys.exit("S = %d, chunks = %d, W = %d: exit status %d" % (S, chunks, W, r.returncode))
                line = r.stdout.strip().splitlines()[-1]
                json.loads(line)
                print(line, flush=True)
                lines.append(line)
                with open(args.out, "w") as fh:
                    fh.write("\n".join(lines) + "\n")
    sys.exit(0)

import numpy as np
import torch
import rustpotter_amd as ra

assert torch.cuda.is_available(), "this measurement needs a GPU"
S, CHUNKS, W = [int(x) for x in args.child.split(",")]
TEMPLATES, MAX_DET = 5, 4
rng = np.random.default_rng(W)


def template(n):
    """a smooth random walk in five coefficients, mean-normalised like the rows of a .rpw"""
    x = np.cumsum(rng.standard_normal((n, 5)), axis=0) + 4.0 * rng.standard_normal((n, 5))
    return (x - x.mean(axis=0)).astype(np.float32)


host = ra.BatchContext(0, host_pointers=True)
ctx = ra.BatchContext(0, host_pointers=False)
words = [[template(int(rng.integers(90, 111))) for _ in range(TEMPLATES)] for _ in range(W)]
avgs = host.average_templates([sorted(ww, key=lambda t: -len(t)) for ww in words])
bank = ra.WakewordBank(ctx, wakewords=[(ww, a, None, None) for ww, a in zip(words, avgs)])
one = ra.Templates(ctx, words[0], avgs[0])
del host
cfg = ra.DetectorConfig()
idx = (torch.arange(S, dtype=torch.int32) % W).cuda()
N = CHUNKS * 480
# a few calls' worth of different audio, reused round after round
f32 = torch.empty((S, 4 * N), dtype=torch.float32, device="cuda")
ctx.synth_dev(0x5EED, 0, S, 4 * N, 4 * N, f32.data_ptr())
pcm = [(f32[:, j * N:(j + 1) * N] * 32767.0).round().clamp(-32768, 32767).to(torch.int16).contiguous() for j in range(4)]
del f32
det = torch.zeros((S, MAX_DET, 6), dtype=torch.int32, device="cuda")
n_det = torch.zeros(S, dtype=torch.int32, device="cuda")
ctx.set_arithmetic("strict_f32")   # the shared batch's arithmetic; a batch over a bank does not read the setting
batches = {"bank": ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=CHUNKS, bank=bank, stream_wakeword=int(idx.data_ptr())),
           "shared": ra.StreamBatch(ctx, one, cfg, S, max_chunks_per_call=CHUNKS)}
count = {"bank": 0, "shared": 0}


def calls(k, n):
    sb = batches[k]
    for _ in range(n):
        sb.process_dev(pcm[count[k] % 4].data_ptr(), 1, CHUNKS, N, det.data_ptr(), n_det.data_ptr(), MAX_DET)
        count[k] += 1
    ctx.synchronize()


# both batches past the point where every stream's window is full (110 frames) before anything is timed
fill = (110 + 3 * CHUNKS - 1) // (3 * CHUNKS) + 1
ctx.dtw_kernels()
kernels = {}
for k in batches:
    calls(k, fill)
    kernels[k] = ctx.dtw_kernels()
for _ in range(2):
    for k in batches:
        calls(k, args.calls)
ms = {"bank": [], "shared": []}
for _ in range(args.repeats):
    for k in batches:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        calls(k, args.calls)
        ms[k].append((time.perf_counter() - t0) * 1e3 / args.calls)
dtw_ms = {}
ctx.timing_enable(True)
for k in batches:
    ctx.timing_reset()
    calls(k, 5)
    avg_ms, launches = ctx.timing_read(1)   # average per timed launch bracket; the shared batch may have several per call
    dtw_ms[k] = round(avg_ms * launches / 5, 4)
ctx.timing_enable(False)
res = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms.items()}
print(json.dumps({
    "metric": "ms per process call: a live-stream batch over a wakeword bank (per-stream wakewords) against the shared-wakeword live batch (strict f32, one wakeword of the same shape)",
    "streams": S, "chunks_per_call": CHUNKS, "wakewords": W, "input": "i16", "templates_per_wakeword": TEMPLATES, "template_frames": "90-110", "mfcc_size": 5, "band": 5,
    "detect_only": True, "rounds": args.repeats, "calls_per_round": args.calls, "ms": res,
    "bank_over_shared": round(res["bank"]["median_ms"] / res["shared"]["median_ms"], 3), "dtw_ms": dtw_ms,
    "dtw_bank_over_shared": round(dtw_ms["bank"] / dtw_ms["shared"], 3) if dtw_ms["shared"] else None, "kernels": kernels,
    "device": torch.cuda.get_device_name(0), "build": ra.build_info()}), flush=True)
