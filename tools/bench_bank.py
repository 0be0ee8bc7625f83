"""Personal wakewords: ONE rp_batch_detect_bank call (stream s carries wakeword s mod W of a bank) against today's only alternative, a loop
of rp_batch_detect under RP_ARITH_STRICT_F32 with one call per wakeword over that wakeword's S / W streams, in one process.  S streams x 4 s
of synthetic PCM on the device, mfcc_size 5, band 5, detect-only; W wakewords of 5 templates of 90-110 frames with an averaged template.
Every W runs in a fresh process under its own time limit; the two forms alternate, two warm-up rounds each, `--repeats` timed rounds
(ten bank calls per round, one pass of the loop), medians in ms per call.  At W = 1 the "loop" is plain rp_batch_detect on the same streams: the ratio is the price of the per-stream indirection.
One JSON line per W; all lines go to --out.
usage: python tools/bench_bank.py [--wakewords 1,64,1024,8192] [--streams 8192] [--repeats 5] [--out profiles/bench_bank.json]"""
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
ap.add_argument("--wakewords", default="1,64,1024,8192")
ap.add_argument("--streams", type=int, default=8192)
ap.add_argument("--seconds", type=float, default=4.0)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--step-timeout", type=int, default=420)
ap.add_argument("--out", default=os.path.join("profiles", "bench_bank.json"))
ap.add_argument("--child", type=int, default=0, help="(internal) measure this W and print its line")
args = ap.parse_args()
assert args.repeats >= 5, "medians over at least five rounds"

if not args.child:
    lines = []
    for W in [int(x) for x in args.wakewords.split(",")]:
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
W, S, TEMPLATES = args.child, args.streams, 5
assert S % W == 0
N = int(args.seconds * 16000) // 480 * 480
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
tmpl = [ra.Templates(ctx, ww, a) for ww, a in zip(words, avgs)]
del host
cfg = ra.DetectorConfig()
MAX_DET = 4
pcm = torch.empty((S, N), dtype=torch.float32, device="cuda")
ctx.synth_dev(0x5EED, 0, S, N, N, pcm.data_ptr())
det = torch.zeros((S, MAX_DET, 6), dtype=torch.int32, device="cuda")
n_det = torch.zeros(S, dtype=torch.int32, device="cuda")
per = S // W
idx_rr = (torch.arange(S, dtype=torch.int32) % W).cuda()       # round-robin: what the timed bank calls use
idx_blk = (torch.arange(S, dtype=torch.int32) // per).cuda()   # wakeword w owns streams w * per ..: what the loop scores


def bank_call(idx):
    ctx.batch_detect_bank_dev(pcm.data_ptr(), 3, S, N, N, bank, idx.data_ptr(), cfg, det.data_ptr(), n_det.data_ptr(), MAX_DET)
    ctx.synchronize()


def loop_call():
    for w in range(W):
        ctx.batch_detect_dev(pcm.data_ptr() + w * per * N * 4, per, N, N, tmpl[w], cfg, det.data_ptr() + w * per * MAX_DET * 24,
                             n_det.data_ptr() + w * per * 4, MAX_DET)
    ctx.synchronize()


ctx.set_arithmetic("strict_f32")   # the loop's arithmetic; bank calls do not read the setting
bank_call(idx_blk)
got = n_det.cpu().numpy().copy()
loop_call()
same = bool(np.array_equal(got, n_det.cpu().numpy()))
ctx.dtw_kernels()
for _ in range(2):
    bank_call(idx_rr)
    loop_call()
kernels = ctx.dtw_kernels()
ms = {"bank": [], "loop": []}
calls = {"bank": 10, "loop": 10 if W == 1 else 1}   # calls per timed window: a window of a few milliseconds measures the scheduler
for _ in range(args.repeats):
    for k, fn in (("bank", lambda: bank_call(idx_rr)), ("loop", loop_call)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _i in range(calls[k]):
            fn()
        ms[k].append((time.perf_counter() - t0) * 1e3 / calls[k])
# the DTW kernel of the bank call alone (kernel 1 of rp_ctx_timing_read)
ctx.timing_enable(True)
ctx.timing_reset()
for _ in range(3):
    bank_call(idx_rr)
dtw_ms = round(ctx.timing_read(1)[0], 4)
ctx.timing_enable(False)
nf = ra.mfcc_num_frames(N)
scorings = float(sum((nf - bank.max_lens[s % W] + 1) * TEMPLATES for s in range(S)))
res = {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in ms.items()}
print(json.dumps({
    "metric": "ms per call: one rp_batch_detect_bank (per-stream wakewords) against a loop of rp_batch_detect (strict f32), one call per wakeword",
    "wakewords": W, "streams": S, "seconds": N / 16000.0, "templates_per_wakeword": TEMPLATES, "template_frames": "90-110", "mfcc_size": 5, "band": 5,
    "detect_only": True, "rounds": args.repeats, "calls_per_round": calls, "ms": res, "loop_over_bank": round(res["loop"]["median_ms"] / res["bank"]["median_ms"], 3),
    "n_det_equal": same, "dtw_bank_kernel_ms": dtw_ms, "sample_template_scorings": scorings, "kernels": kernels,
    "device": torch.cuda.get_device_name(0), "build": ra.build_info()}), flush=True)
