"""Personal wakeword models: ONE rp_batch_detect_model_bank call (stream s is run by model s mod W of a model bank) against
(a) "shared": one rp_batch_detect_model over all streams with ONE shared model -- what per-stream weights cost, and
(b) "loop": a loop of rp_batch_detect_model, one call per model over that model's S / W streams -- the route there was before the bank,
in one process.  S streams x 4 s of synthetic PCM on the device, mfcc_size 16; W random Small models of 195 frames (195 * 16 -> 32 -> 16 -> 2),
RP_MLP_F32.  Every W runs in a fresh process under its own time limit; the three forms alternate, two warm-up rounds each, `--repeats`
timed rounds, medians in ms per call.  At W = 1 the loop is the shared call.
One JSON line per W; all lines go to --out.
usage: python tools/bench_model_bank.py [--models 1,64,1024] [--streams 8192] [--repeats 5] [--out profiles/bench_model_bank.json]"""
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
ap.add_argument("--models", default="1,64,1024")
ap.add_argument("--streams", type=int, default=8192)
ap.add_argument("--seconds", type=float, default=4.0)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=os.path.join("profiles", "bench_model_bank.json"))
ap.add_argument("--child", type=int, default=0, help="(internal) measure this W and print its line")
args = ap.parse_args()
assert args.repeats >= 5, "medians over at least five rounds"

if not args.child:
    lines = []
    for W in [int(x) for x in args.models.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", str(W), "--streams", str(args.streams),
               "--seconds", str(args.seconds), "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:   # nothing more is started on the device after a step that failed
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("W = %d: exit status %d" % (W, r.returncode))
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
W, S, K, L = args.child, args.streams, 16, 195
assert S % W == 0
N = int(args.seconds * 16000) // 480 * 480
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
MAX_DET = 4
pcm = torch.empty((S, N), dtype=torch.float32, device="cuda")
ctx.synth_dev(0x5EED, 0, S, N, N, pcm.data_ptr())
det = torch.zeros((S, MAX_DET, 6), dtype=torch.int32, device="cuda")
lab = torch.zeros((S, MAX_DET), dtype=torch.int32, device="cuda")
n_det = torch.zeros(S, dtype=torch.int32, device="cuda")
per = S // W
idx_rr = (torch.arange(S, dtype=torch.int32) % W).cuda()       # round-robin: what the timed bank calls use
idx_blk = (torch.arange(S, dtype=torch.int32) // per).cuda()   # model w owns streams w * per ..: what the loop runs


def bank_call(idx):
    ctx.batch_detect_model_bank_dev(pcm.data_ptr(), 3, S, N, N, bank, idx.data_ptr(), cfg, "f32", det.data_ptr(), lab.data_ptr(), n_det.data_ptr(), MAX_DET)
    ctx.synchronize()


def shared_call():
    ctx.batch_detect_model_dev(pcm.data_ptr(), 3, S, N, N, models[0], K, 0, cfg, "f32", det.data_ptr(), lab.data_ptr(), n_det.data_ptr(), MAX_DET)
    ctx.synchronize()


def loop_call():
    for w in range(W):
        ctx.batch_detect_model_dev(pcm.data_ptr() + w * per * N * 4, 3, per, N, N, models[w], K, 0, cfg, "f32", det.data_ptr() + w * per * MAX_DET * 24,
                                   lab.data_ptr() + w * per * MAX_DET * 4, n_det.data_ptr() + w * per * 4, MAX_DET)
    ctx.synchronize()


bank_call(idx_blk)
bank_kernel = ctx.last_mlp_kernel()
got = (n_det.cpu().numpy().copy(), det.cpu().numpy().copy())
loop_call()
loop_kernel = ctx.last_mlp_kernel()
# frame, window, counter and the bits of both scores; a detection's stream number counts within its call
same = bool(np.array_equal(got[0], n_det.cpu().numpy()) and np.array_equal(got[1][:, :, 1:], det.cpu().numpy()[:, :, 1:]))
n_detections = int(np.minimum(got[0], MAX_DET).sum())
forms = (("bank", lambda: bank_call(idx_rr)), ("shared", shared_call), ("loop", loop_call))
for _ in range(2):
    for _k, fn in forms:
        fn()
ms = {"bank": [], "shared": [], "loop": []}
calls = {"bank": 5, "shared": 5, "loop": 5 if W == 1 else 1}   # calls per timed window
for _ in range(args.repeats):
    for k, fn in forms:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _i in range(calls[k]):
            fn()
        ms[k].append((time.perf_counter() - t0) * 1e3 / calls[k])
# the forward kernels alone (kernel 4 of rp_ctx_timing_read)
ctx.timing_enable(True)
kernel_ms = {}
for k, fn in forms[:2]:
    ctx.timing_reset()
    for _ in range(3):
        fn()
    kernel_ms[k] = round(ctx.timing_read(4)[0], 4)
ctx.timing_enable(False)
res = {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in ms.items()}
nf = ra.mfcc_num_frames(N)
print(json.dumps({
    "metric": "ms per call: one rp_batch_detect_model_bank (per-stream models) against one rp_batch_detect_model with a shared model and against a loop of rp_batch_detect_model, one call per model",
    "models": W, "streams": S, "seconds": N / 16000.0, "model": "Small, 195 frames x 16 -> 32 -> 16 -> 2", "windows_per_stream": nf - L + 1,
    "layer1_image_bytes_per_model": L * 3072, "precision": "RP_MLP_F32", "rounds": args.repeats, "calls_per_round": calls, "ms": res,
    "bank_over_shared": round(res["bank"]["median_ms"] / res["shared"]["median_ms"], 3),
    "loop_over_bank": round(res["loop"]["median_ms"] / res["bank"]["median_ms"], 3),
    "detections_equal_bank_vs_loop": same, "detections_compared": n_detections, "forward_kernel_ms": kernel_ms, "kernels": {"bank": bank_kernel, "loop": loop_kernel},
    "device": torch.cuda.get_device_name(0), "build": ra.build_info()}), flush=True)
