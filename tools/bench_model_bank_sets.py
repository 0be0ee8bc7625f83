"""Model sets (several models of a model bank per stream) against what a caller can do without them, in one process:
  whole: one rp_batch_detect_model_bank_sets call over S streams of 4 s against set_size calls of rp_batch_detect_model_bank, one per slot;
  live:  one live-stream batch over model sets (rp_stream_batch_new_model_bank_sets) against set_size live-stream batches over the model
         bank, fed `chunks` 30 ms chunks per call.
The baseline does NOT give the right detections (it is set_size independent detectors, each with its own window, countdown and partial
detection): it is the cost yardstick only, and no ratio is a pass condition.  The forward reads one layer-1 image per live slot on both
sides; what a set saves is the front end, the MFCC and the scan.  Synthetic i16 PCM from the device, W = 64 Small models of 195 frames
(32 and 16 hidden units, two labels); stream s holds models (s + 17 j) mod W, j < set_size.  Every case runs in a fresh process under its own
time limit; the two sides alternate, two warm-up rounds each, `--repeats` timed rounds, medians in ms per call.  One JSON line per case; all
lines go to --out.
usage: python tools/bench_model_bank_sets.py [--set-sizes 2,4] [--streams 8192] [--chunks 1,8] [--repeats 5] [--out profiles/bench_model_bank_sets.json]"""
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
ap.add_argument("--set-sizes", default="2,4")
ap.add_argument("--streams", default="8192", help="live cases; the whole-recording case runs at --whole-streams")
ap.add_argument("--whole-streams", type=int, default=8192)
ap.add_argument("--chunks", default="1,8")
ap.add_argument("--models", type=int, default=64)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=20, help="process calls per timed round (live)")
ap.add_argument("--step-timeout", type=int, default=240)
ap.add_argument("--out", default=os.path.join("profiles", "bench_model_bank_sets.json"))
ap.add_argument("--child", default="", help="(internal) whole,S,set_size or live,S,chunks,set_size: measure this case and print its line")
args = ap.parse_args()
assert args.repeats >= 5, "medians over at least five rounds"

if not args.child:
    cases = []
    for n in [int(x) for x in args.set_sizes.split(",")]:
        cases.append("whole,%d,%d" % (args.whole_streams, n))
        for S in [int(x) for x in args.streams.split(",")]:
            for chunks in [int(x) for x in args.chunks.split(",")]:
                cases.append("live,%d,%d,%d" % (S, chunks, n))
    lines = []
    for case in cases:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", case, "--repeats", str(args.repeats),
               "--calls", str(args.calls), "--models", str(args.models)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:   # nothing more is started on the device after a step that failed
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("%s: exit status %d" % (case, r.returncode))
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
kind, *nums = args.child.split(",")
nums = [int(x) for x in nums]
W, L, MAX_DET = args.models, 195, 4
rng = np.random.default_rng(W)
ctx = ra.BatchContext(0, host_pointers=False)
dims = [L * 16, 32, 16, 2]


def small_model():
    ws = [(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32) for i in range(3)]
    bs = [(rng.standard_normal(dims[i + 1]) * 0.1).astype(np.float32) for i in range(3)]
    return ra.Model(ctx, ws, bs)


bank = ra.ModelBank(ctx, models=[small_model() for _ in range(W)], none_index=[0] * W)
cfg = ra.DetectorConfig()
S, SET = nums[0], nums[-1]
sets = ((torch.arange(S, dtype=torch.int32)[:, None] + 17 * torch.arange(SET, dtype=torch.int32)[None, :]) % W).contiguous().cuda()
cols = [sets[:, j].contiguous() for j in range(SET)]   # the baseline's indices: one array per slot
det = torch.zeros((S, MAX_DET, 6), dtype=torch.int32, device="cuda")
det_ww = torch.zeros((S, MAX_DET), dtype=torch.int32, device="cuda")
det_label = torch.zeros((S, MAX_DET), dtype=torch.int32, device="cuda")
n_det = torch.zeros(S, dtype=torch.int32, device="cuda")
common = {"streams": S, "set_size": SET, "models": W, "input": "i16", "model": "Small, 195 frames, 32 / 16 hidden units, 2 labels", "mfcc_size": 16,
          "rounds": args.repeats, "baseline_gives_the_right_detections": False}


def to_i16(x):
    return (x * 32767.0).round().clamp(-32768, 32767).to(torch.int16).contiguous()


def medians(run, calls_per_round):
    """run[k](): one round of side k; the sides alternate, two warm-up rounds each"""
    for _ in range(2):
        for k in run:
            run[k]()
    ms = {k: [] for k in run}
    for _ in range(args.repeats):
        for k in run:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run[k]()
            ms[k].append((time.perf_counter() - t0) * 1e3 / calls_per_round)
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms.items()}


if kind == "whole":
    N = 480 * 133   # 4 s
    f32 = torch.empty((S, N), dtype=torch.float32, device="cuda")
    ctx.synth_dev(0x5EED, 0, S, N, N, f32.data_ptr())
    pcm = to_i16(f32)
    del f32

    def sets_call():
        ctx.batch_detect_model_bank_sets_dev(pcm.data_ptr(), 1, S, N, N, bank, sets.data_ptr(), SET, cfg, "f32", det.data_ptr(), det_ww.data_ptr(),
                                             det_label.data_ptr(), n_det.data_ptr(), MAX_DET)
        ctx.synchronize()

    def bank_calls():
        for c in cols:
            ctx.batch_detect_model_bank_dev(pcm.data_ptr(), 1, S, N, N, bank, c.data_ptr(), cfg, "f32", det.data_ptr(), det_label.data_ptr(),
                                            n_det.data_ptr(), MAX_DET)
        ctx.synchronize()

    res = medians({"sets": sets_call, "bank_calls": bank_calls}, 1)
    print(json.dumps(dict(common, metric="ms: one rp_batch_detect_model_bank_sets call against set_size rp_batch_detect_model_bank calls, one per slot (whole recordings of 4 s)",
                          ms=res, sets_over_bank_calls=round(res["sets"]["median_ms"] / res["bank_calls"]["median_ms"], 3),
                          device=torch.cuda.get_device_name(0), build=ra.build_info())), flush=True)
else:
    CHUNKS = nums[1]
    N = CHUNKS * 480
    f32 = torch.empty((S, 4 * N), dtype=torch.float32, device="cuda")
    ctx.synth_dev(0x5EED, 0, S, 4 * N, 4 * N, f32.data_ptr())
    pcm = [to_i16(f32[:, j * N:(j + 1) * N]) for j in range(4)]   # a few calls' worth of different audio, reused round after round
    del f32
    one = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=CHUNKS, model_bank=bank, stream_models=int(sets.data_ptr()), set_size=SET)
    many = [ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=CHUNKS, model_bank=bank, stream_model=int(c.data_ptr())) for c in cols]
    count = {"sets": 0, "bank_batches": 0}

    def calls(k, n):
        for _ in range(n):
            p = pcm[count[k] % 4].data_ptr()
            for sb in ([one] if k == "sets" else many):
                sb.process_dev(p, 1, CHUNKS, N, det.data_ptr(), n_det.data_ptr(), MAX_DET)
            count[k] += 1
        ctx.synchronize()

    # both sides past the point where every stream's window is full (195 frames) before anything is timed
    fill = (L + 3 * CHUNKS - 1) // (3 * CHUNKS) + 1
    for k in count:
        calls(k, fill)
    res = medians({k: (lambda k=k: calls(k, args.calls)) for k in count}, args.calls)
    print(json.dumps(dict(common, metric="ms per step of `chunks_per_call` chunks: one live-stream batch over model sets against set_size live-stream batches over the model bank",
                          chunks_per_call=CHUNKS, calls_per_round=args.calls, ms=res,
                          sets_over_bank_batches=round(res["sets"]["median_ms"] / res["bank_batches"]["median_ms"], 3),
                          device=torch.cuda.get_device_name(0), build=ra.build_info())), flush=True)
