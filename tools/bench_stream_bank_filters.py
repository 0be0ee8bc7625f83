"""What the per-stream gain normaliser costs a live-stream batch over a wakeword bank (rp_stream_batch_set_filters_bank: stream s works
towards the rms_level of wakeword s mod W over that wakeword's own window): the bank batch with gain normaliser + band-pass against
(a) the same bank batch with the band-pass alone (rp_stream_batch_set_filters) and (b) the shared-wakeword live batch (rp_stream_batch_new
under RP_ARITH_STRICT_F32, ONE wakeword of the same shape) with both filters -- the one window and level of stream_filters_kernel's shared form.
S streams fed `chunks` 30 ms chunks of i16 noise per call from the device (every stream at its own loudness, so the gains are not all alike),
mfcc_size 5, band 5, detect-only; W wakewords of 5 templates of 90-110 frames with rms_level spread over 0.01-0.06.  Every (S, chunks) runs in
a fresh process under its own time limit; the three batches alternate, two warm-up rounds each, `--repeats` timed rounds of `--calls` process
calls, medians in ms per call.  One JSON line per case; all lines go to --out.
usage: python tools/bench_stream_bank_filters.py [--streams 8192,65536] [--chunks 1,8] [--wakewords 64] [--repeats 5] [--out profiles/bench_stream_bank_filters.json]"""
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
ap.add_argument("--wakewords", type=int, default=64)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=20, help="process calls per timed round")
ap.add_argument("--step-timeout", type=int, default=240)
ap.add_argument("--out", default=os.path.join("profiles", "bench_stream_bank_filters.json"))
ap.add_argument("--child", default="", help="(internal) S,chunks: measure this case and print its line")
args = ap.parse_args()
assert args.repeats >= 5, "medians over at least five rounds"

if not args.child:
    lines = []
    for S in [int(x) for x in args.streams.split(",")]:
        for chunks in [int(x) for x in args.chunks.split(",")]:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "%d,%d" % (S, chunks),
                   "--wakewords", str(args.wakewords), "--repeats", str(args.repeats), "--calls", str(args.calls)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:   # nothing more is started on the device after a step that failed
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit("S = %d, chunks = %d: exit status %d" % (S, chunks, r.returncode))
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
S, CHUNKS = [int(x) for x in args.child.split(",")]
W, TEMPLATES, MAX_DET = args.wakewords, 5, 4
rng = np.random.default_rng(W)


def template(n):
    """a smooth random walk in five coefficients, mean-normalised like the rows of a .rpw"""
    x = np.cumsum(rng.standard_normal((n, 5)), axis=0) + 4.0 * rng.standard_normal((n, 5))
    return (x - x.mean(axis=0)).astype(np.float32)


def filters(gain, band):
    f = ra.FiltersConfig()
    f.gain_normalizer.enabled, f.gain_normalizer.min_gain, f.gain_normalizer.max_gain = gain, 0.2, 3.0
    f.band_pass.enabled, f.band_pass.low_cutoff, f.band_pass.high_cutoff = band, 120.0, 900.0
    return f


host = ra.BatchContext(0, host_pointers=True)
ctx = ra.BatchContext(0, host_pointers=False)
words = [[template(int(rng.integers(90, 111))) for _ in range(TEMPLATES)] for _ in range(W)]
avgs = host.average_templates([sorted(ww, key=lambda t: -len(t)) for ww in words])
bank = ra.WakewordBank(ctx, wakewords=[(ww, a, None, None) for ww, a in zip(words, avgs)])
levels = np.linspace(0.01, 0.06, W).astype(np.float32)
bank.set_rms_levels(levels)
one = ra.Templates(ctx, words[0], avgs[0])
del host
cfg = ra.DetectorConfig()
idx = (torch.arange(S, dtype=torch.int32) % W).cuda()
N = CHUNKS * 480
# a few calls' worth of noise, every stream at its own loudness, reused round after round
amp = torch.exp(torch.empty((S, 1), device="cuda").uniform_(float(np.log(0.01)), float(np.log(0.6))))
pcm = [((torch.randn((S, N), device="cuda") * amp).clamp_(-1.0, 1.0) * 32767.0).round().to(torch.int16).contiguous() for _ in range(4)]
det = torch.zeros((S, MAX_DET, 6), dtype=torch.int32, device="cuda")
n_det = torch.zeros(S, dtype=torch.int32, device="cuda")
ctx.set_arithmetic("strict_f32")   # the shared batch's arithmetic; a batch over a bank does not read the setting
bank_kw = dict(max_chunks_per_call=CHUNKS, bank=bank, stream_wakeword=int(idx.data_ptr()))
batches = {"bank_gain_band_pass": ra.StreamBatch(ctx, None, cfg, S, bank_filters=filters(True, True), **bank_kw),
           "bank_band_pass": ra.StreamBatch(ctx, None, cfg, S, filters=filters(False, True), **bank_kw),
           "shared_gain_band_pass": ra.StreamBatch(ctx, one, cfg, S, max_chunks_per_call=CHUNKS, filters=filters(True, True), rms_level_ref=float(levels[0]))}
count = {k: 0 for k in batches}


def calls(k, n):
    sb = batches[k]
    for _ in range(n):
        sb.process_dev(pcm[count[k] % 4].data_ptr(), 1, CHUNKS, N, det.data_ptr(), n_det.data_ptr(), MAX_DET)
        count[k] += 1
    ctx.synchronize()


# every batch past the point where every stream's MFCC window (110 frames) and gain window (36 levels) is full before anything is timed
fill = max((110 + 3 * CHUNKS - 1) // (3 * CHUNKS) + 1, -(-37 // CHUNKS))
for k in batches:
    calls(k, fill)
for _ in range(2):
    for k in batches:
        calls(k, args.calls)
ms = {k: [] for k in batches}
for _ in range(args.repeats):
    for k in batches:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        calls(k, args.calls)
        ms[k].append((time.perf_counter() - t0) * 1e3 / args.calls)
res = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms.items()}
m = lambda k: res[k]["median_ms"]
print(json.dumps({
    "metric": "ms per process call: a live-stream batch over a wakeword bank with the per-stream gain normaliser + band-pass, against the same batch with "
              "the band-pass alone and against the shared-wakeword live batch (strict f32, one wakeword of the same shape) with both filters",
    "streams": S, "chunks_per_call": CHUNKS, "wakewords": W, "rms_levels": "0.01-0.06", "input": "i16", "templates_per_wakeword": TEMPLATES,
    "template_frames": "90-110", "mfcc_size": 5, "band": 5, "detect_only": True, "rounds": args.repeats, "calls_per_round": args.calls, "ms": res,
    "over_bank_band_pass": round(m("bank_gain_band_pass") / m("bank_band_pass"), 3),
    "over_shared_gain_band_pass": round(m("bank_gain_band_pass") / m("shared_gain_band_pass"), 3),
    "device": torch.cuda.get_device_name(0), "build": ra.build_info()}), flush=True)
