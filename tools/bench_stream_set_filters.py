"""What the gain normaliser costs the live-stream batches whose streams hold a SET of bank entries or a model
(rp_stream_batch_set_filters_per_stream: stream_targets_kernel folds every stream's row into a level and a window at the start of each call,
then the per-stream form of stream_filters_kernel): a wakeword-sets batch, a model-bank batch and a model-sets batch with gain normaliser +
band-pass, each against the SAME batch with the band-pass alone (rp_stream_batch_set_filters), the path that existed before.
S streams fed `chunks` 30 ms chunks of i16 noise per call from the device (every stream at its own loudness, so the gains are not all
alike), detect-only; W wakewords of 5 templates of 90-110 frames (mfcc_size 5, band 5) and W Tiny models of 90-110 frames, levels spread over
0.01-0.06; stream s holds entries s, s + 1, ... mod W.  Every (S, chunks, set_size) runs in a fresh process under its own time limit; the
six batches alternate, two warm-up rounds each, `--repeats` timed rounds of `--calls` process calls, medians in ms per call.  One JSON line
per case; all lines go to --out.
usage: python tools/bench_stream_set_filters.py [--streams 8192,65536] [--chunks 1,8] [--set-sizes 1,2,4] [--wakewords 64] [--repeats 5]
       [--out profiles/bench_stream_set_filters.json]"""
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
ap.add_argument("--set-sizes", default="1,2,4")
ap.add_argument("--wakewords", type=int, default=64)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=20, help="process calls per timed round")
ap.add_argument("--step-timeout", type=int, default=240)
ap.add_argument("--out", default=os.path.join("profiles", "bench_stream_set_filters.json"))
ap.add_argument("--child", default="", help="(internal) S,chunks,set_size: measure this case and print its line")
args = ap.parse_args()
assert args.repeats >= 5, "medians over at least five rounds"

if not args.child:
    lines = []
    for S in [int(x) for x in args.streams.split(",")]:
        for chunks in [int(x) for x in args.chunks.split(",")]:
            for n in [int(x) for x in args.set_sizes.split(",")]:
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "%d,%d,%d" % (S, chunks, n),
                       "--wakewords", str(args.wakewords), "--repeats", str(args.repeats), "--calls", str(args.calls)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:   # nothing more is started on the device after a step that failed
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    sys.exit("S = %d, chunks = %d, set_size = %d: exit status %d" % (S, chunks, n, r.returncode))
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
S, CHUNKS, SET = [int(x) for x in args.child.split(",")]
W, TEMPLATES, MAX_DET, HIDDEN = args.wakewords, 5, 4, 8
rng = np.random.default_rng(W)


def template(n):
    """a smooth random walk in five coefficients, mean-normalised like the rows of a .rpw"""
    x = np.cumsum(rng.standard_normal((n, 5)), axis=0) + 4.0 * rng.standard_normal((n, 5))
    return (x - x.mean(axis=0)).astype(np.float32)


def tiny(n):
    """a random Tiny model of n frames: (weights, biases)"""
    dims = [n * 16, HIDDEN, 2]
    return ([(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32) for i in range(2)],
            [(rng.standard_normal(dims[i + 1]) * 0.1).astype(np.float32) for i in range(2)])


def filters(gain, band):
    f = ra.FiltersConfig()
    f.gain_normalizer.enabled, f.gain_normalizer.min_gain, f.gain_normalizer.max_gain = gain, 0.2, 3.0
    f.band_pass.enabled, f.band_pass.low_cutoff, f.band_pass.high_cutoff = band, 120.0, 900.0
    return f


host = ra.BatchContext(0, host_pointers=True)
ctx = ra.BatchContext(0, host_pointers=False)
words = [[template(int(rng.integers(90, 111))) for _ in range(TEMPLATES)] for _ in range(W)]
avgs = host.average_templates([sorted(ww, key=lambda t: -len(t)) for ww in words])
del host
levels = np.linspace(0.01, 0.06, W).astype(np.float32)
bank = ra.WakewordBank(ctx, wakewords=[(ww, a, None, None) for ww, a in zip(words, avgs)])
bank.set_rms_levels(levels)
models = [ra.Model(ctx, *tiny(int(rng.integers(90, 111)))) for _ in range(W)]
mbank = ra.ModelBank(ctx, models=models, none_index=[0] * W)
mbank.set_rms_levels(levels)
del models
cfg = ra.DetectorConfig()
one = (torch.arange(S, dtype=torch.int32) % W).cuda()
rows = ((torch.arange(S, dtype=torch.int32)[:, None] + torch.arange(SET, dtype=torch.int32)[None, :]) % W).contiguous().cuda()
N = CHUNKS * 480
# a few calls' worth of noise, every stream at its own loudness, reused round after round
amp = torch.exp(torch.empty((S, 1), device="cuda").uniform_(float(np.log(0.01)), float(np.log(0.6))))
pcm = [((torch.randn((S, N), device="cuda") * amp).clamp_(-1.0, 1.0) * 32767.0).round().to(torch.int16).contiguous() for _ in range(4)]
det = torch.zeros((S, MAX_DET, 6), dtype=torch.int32, device="cuda")
n_det = torch.zeros(S, dtype=torch.int32, device="cuda")
kinds = {"sets": dict(bank=bank, stream_wakewords=int(rows.data_ptr()), set_size=SET),
         "model_bank": dict(model_bank=mbank, stream_model=int(one.data_ptr())),
         "model_sets": dict(model_bank=mbank, stream_models=int(rows.data_ptr()), set_size=SET)}
batches = {}
for k, kw in kinds.items():
    batches[k + "_gain_band_pass"] = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=CHUNKS, per_stream_filters=filters(True, True), **kw)
    batches[k + "_band_pass"] = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=CHUNKS, filters=filters(False, True), **kw)
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
    "metric": "ms per process call: live-stream batches over wakeword sets, a model bank (one model a stream, whatever set_size) and model sets with "
              "the per-stream gain normaliser + band-pass (rp_stream_batch_set_filters_per_stream), each against the same batch with the band-pass alone",
    "streams": S, "chunks_per_call": CHUNKS, "set_size": SET, "entries": W, "rms_levels": "0.01-0.06", "input": "i16",
    "templates_per_wakeword": TEMPLATES, "frames": "90-110", "mfcc_size": {"wakewords": 5, "models": 16}, "band": 5, "detect_only": True,
    "rounds": args.repeats, "calls_per_round": args.calls, "ms": res,
    "over_band_pass": {k: round(m(k + "_gain_band_pass") / m(k + "_band_pass"), 3) for k in kinds},
    "device": torch.cuda.get_device_name(0), "build": ra.build_info()}), flush=True)
