"""Personal wakeword models on live streams: a live-stream batch over a model bank (rp_stream_batch_new_model_bank: stream s runs model s mod W)
against the shared-model live batch (rp_stream_batch_new_multi with ONE model of the same shape), the cost yardstick, and -- for W = 1 and
64 -- against the route there was: W shared-model batches over S / W streams each, one process call per model.  In one process per case:
S streams fed `chunks` 30 ms chunks of synthetic i16 PCM per call from the device, mfcc_size 16, W random Small models of 195 frames
(195 * 16 -> 32 -> 16 -> 2), RP_MLP_F32.  The routes alternate, two warm-up rounds each, `--repeats` timed rounds of `--calls` process calls,
medians in ms per call.  Also the forward kernel of a call alone (kernel 4 of rp_ctx_timing_read) and the layer-1 image bytes a call of the
bank batch reads, sum over streams of L(s) * 3 072, over that time -- against the 8 TB/s HBM peak (streams that share a model may be served
from the caches, so the figure can exceed what HBM delivers).  One JSON line per case; all lines go to --out.
usage: python tools/bench_stream_model_bank.py [--streams 8192] [--chunks 1,8] [--models 1,64,1024] [--repeats 5] [--out profiles/bench_stream_model_bank.json]"""
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
ap.add_argument("--streams", type=int, default=8192)
ap.add_argument("--chunks", default="1,8")
ap.add_argument("--models", default="1,64,1024")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=20, help="process calls per timed round")
ap.add_argument("--loop-up-to", type=int, default=64, help="the largest W for which the one-batch-per-model route is measured")
ap.add_argument("--step-timeout", type=int, default=240)
ap.add_argument("--out", default=os.path.join("profiles", "bench_stream_model_bank.json"))
ap.add_argument("--child", default="", help="(internal) chunks,W: measure this case and print its line")
args = ap.parse_args()
assert args.repeats >= 5, "medians over at least five rounds"

if not args.child:
    lines = []
    for chunks in [int(x) for x in args.chunks.split(",")]:
        for W in [int(x) for x in args.models.split(",")]:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "%d,%d" % (chunks, W),
                   "--streams", str(args.streams), "--repeats", str(args.repeats), "--calls", str(args.calls), "--loop-up-to", str(args.loop_up_to)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:   # nothing more is started on the device after a step that failed
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit("chunks = %d, W = %d: exit status %d" % (chunks, W, r.returncode))
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
CHUNKS, W = [int(x) for x in args.child.split(",")]
S, K, L, MAX_DET = args.streams, 16, 195, 4
assert S % W == 0
rng = np.random.default_rng(W)
DIMS = (L * K, 32, 16, 2)


def small_model():
    ws = [(rng.standard_normal((DIMS[i + 1], DIMS[i]), dtype=np.float32) / np.float32(np.sqrt(DIMS[i]))) for i in range(3)]
    bs = [rng.standard_normal(DIMS[i + 1], dtype=np.float32) * np.float32(0.1) for i in range(3)]
    return ra.Model(ctx, ws, bs)


ctx = ra.BatchContext(0, host_pointers=False)
models = [small_model() for _ in range(W)]
bank = ra.ModelBank(ctx, models=models, none_index=[0] * W)
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
torch.cuda.synchronize()


def shared(model, streams):
    return ra.StreamBatch(ctx, None, cfg, streams, max_chunks_per_call=CHUNKS, wakewords=[{"model": model, "none_index": 0}], mfcc_size=K)


# a route = the batches one "call" goes through, each over its own share of the streams
routes = {"bank": [ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=CHUNKS, model_bank=bank, stream_model=int(idx.data_ptr()))],
          "shared": [shared(models[0], S)]}
if W <= args.loop_up_to:
    routes["loop"] = [shared(models[w], S // W) for w in range(W)]
count = {k: 0 for k in routes}


def calls(k, n):
    per = S // len(routes[k])
    for _ in range(n):
        p = pcm[count[k] % 4]
        for j, sb in enumerate(routes[k]):
            sb.process_dev(p.data_ptr() + 2 * j * per * N, 1, CHUNKS, N, det.data_ptr() + 24 * j * per * MAX_DET, n_det.data_ptr() + 4 * j * per, MAX_DET)
        count[k] += 1
    ctx.synchronize()


# every route past the point where every stream's window is full before anything is timed
fill = (L + 3 * CHUNKS - 1) // (3 * CHUNKS) + 1
for k in routes:
    calls(k, fill)
for _ in range(2):
    for k in routes:
        calls(k, args.calls)
ms = {k: [] for k in routes}
for _ in range(args.repeats):
    for k in routes:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        calls(k, args.calls)
        ms[k].append((time.perf_counter() - t0) * 1e3 / args.calls)
fwd_ms = {}
ctx.timing_enable(True)
for k in routes:
    ctx.timing_reset()
    calls(k, 5)
    avg_ms, launches = ctx.timing_read(4)   # average per timed forward bracket; the loop has W per call
    fwd_ms[k] = round(avg_ms * launches / 5, 4)
ctx.timing_enable(False)
res = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms.items()}
image_bytes = S * L * 3072
out = {
    "metric": "ms per process call: a live-stream batch over a model bank (per-stream models) against the shared-model live batch (one model of the same shape) and against one shared-model batch per model",
    "streams": S, "chunks_per_call": CHUNKS, "models": W, "input": "i16", "model": "Small, 195 frames x 16 -> 32 -> 16 -> 2", "mfcc_size": K,
    "rounds": args.repeats, "calls_per_round": args.calls, "ms": res,
    "bank_over_shared": round(res["bank"]["median_ms"] / res["shared"]["median_ms"], 3),
    "loop_over_bank": round(res["loop"]["median_ms"] / res["bank"]["median_ms"], 3) if "loop" in res else None,
    "forward_ms": fwd_ms, "layer1_image_bytes_per_call": image_bytes,
    "layer1_image_tb_per_s": round(image_bytes / (fwd_ms["bank"] * 1e-3) / 1e12, 3) if fwd_ms["bank"] else None,
    "hbm_peak_tb_per_s": 8.0,
    "device": torch.cuda.get_device_name(0), "build": ra.build_info()}
out["layer1_image_over_hbm_peak"] = round(out["layer1_image_tb_per_s"] / 8.0, 3) if out["layer1_image_tb_per_s"] else None
print(json.dumps(out), flush=True)
