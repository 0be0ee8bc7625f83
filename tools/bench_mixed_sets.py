"""Mixed sets (wakeword references of a wakeword bank AND models of a model bank on one stream) against what a caller can do without them,
in one process:
  whole: one rp_batch_detect_mixed_sets call over S streams of 4 s against one rp_batch_detect_bank_sets call plus one
         rp_batch_detect_model_bank_sets call over the same streams;
  live:  one live-stream batch over mixed sets (rp_stream_batch_new_mixed_sets) against one batch over wakeword sets plus one over model sets,
         fed `chunks` 30 ms chunks per call.
The pair does NOT give the right detections (two detectors, each with its own window, countdown and partial detection): it is the cost
yardstick only, and no ratio is a pass condition.  Both sides score every slot once; what the mixed call should save is one front end, one
MFCC pass and one scan.  Synthetic i16 PCM from the device, mfcc_size 16; W = 64 references of five templates of 90 - 110 frames with their
average, W = 64 Small models of 195 frames (32 and 16 hidden units, two labels); stream s holds references and models (s + 17 j) mod W,
j < slots per side.  Every case runs in a fresh process under its own time limit; the two sides alternate, two warm-up rounds each,
`--repeats` timed rounds, medians in ms per call.  One JSON line per case; all lines go to --out.
usage: python tools/bench_mixed_sets.py [--slots 1,2] [--streams 8192] [--chunks 1,8] [--repeats 5] [--out profiles/bench_mixed_sets.json]"""
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
ap.add_argument("--slots", default="1,2", help="slots per side")
ap.add_argument("--streams", default="8192", help="live cases; the whole-recording case runs at --whole-streams")
ap.add_argument("--whole-streams", type=int, default=8192)
ap.add_argument("--chunks", default="1,8")
ap.add_argument("--entries", type=int, default=64, help="references in the wakeword bank and models in the model bank")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=20, help="process calls per timed round (live)")
ap.add_argument("--step-timeout", type=int, default=240)
ap.add_argument("--out", default=os.path.join("profiles", "bench_mixed_sets.json"))
ap.add_argument("--child", default="", help="(internal) whole,S,slots or live,S,chunks,slots: measure this case and print its line")
args = ap.parse_args()
assert args.repeats >= 5, "medians over at least five rounds"

if not args.child:
    cases = []
    for n in [int(x) for x in args.slots.split(",")]:
        cases.append("whole,%d,%d" % (args.whole_streams, n))
        for S in [int(x) for x in args.streams.split(",")]:
            for chunks in [int(x) for x in args.chunks.split(",")]:
                cases.append("live,%d,%d,%d" % (S, chunks, n))
    lines = []
    for case in cases:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", case, "--repeats", str(args.repeats),
               "--calls", str(args.calls), "--entries", str(args.entries)]
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
W, L, TEMPLATES, MAX_DET = args.entries, 195, 5, 4
rng = np.random.default_rng(W)
host = ra.BatchContext(0, host_pointers=True)
ctx = ra.BatchContext(0, host_pointers=False)
dims = [L * 16, 32, 16, 2]


def template(n):
    """a smooth random walk in sixteen coefficients, mean-normalised like the rows of a .rpw"""
    x = np.cumsum(rng.standard_normal((n, 16)), axis=0) + 4.0 * rng.standard_normal((n, 16))
    return (x - x.mean(axis=0)).astype(np.float32)


def small_model():
    ws = [(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32) for i in range(3)]
    bs = [(rng.standard_normal(dims[i + 1]) * 0.1).astype(np.float32) for i in range(3)]
    return ra.Model(ctx, ws, bs)


words = [[template(int(rng.integers(90, 111))) for _ in range(TEMPLATES)] for _ in range(W)]
avgs = host.average_templates([sorted(ww, key=lambda t: -len(t)) for ww in words])
bank = ra.WakewordBank(ctx, wakewords=[(ww, a, None, None) for ww, a in zip(words, avgs)])
del host
mbank = ra.ModelBank(ctx, models=[small_model() for _ in range(W)], none_index=[0] * W)
cfg = ra.DetectorConfig()
S, SET = nums[0], nums[-1]
rows = ((torch.arange(S, dtype=torch.int32)[:, None] + 17 * torch.arange(SET, dtype=torch.int32)[None, :]) % W).contiguous().cuda()
mrows = rows.clone()
det = torch.zeros((S, MAX_DET, 6), dtype=torch.int32, device="cuda")
det_ww = torch.zeros((S, MAX_DET), dtype=torch.int32, device="cuda")
det_label = torch.zeros((S, MAX_DET), dtype=torch.int32, device="cuda")
n_det = torch.zeros(S, dtype=torch.int32, device="cuda")
common = {"streams": S, "slots_per_side": SET, "references": W, "models": W, "input": "i16", "templates_per_reference": TEMPLATES,
          "template_frames": "90-110", "model": "Small, 195 frames, 32 / 16 hidden units, 2 labels", "mfcc_size": 16, "rounds": args.repeats,
          "baseline_gives_the_right_detections": False}


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

    def mixed_call():
        ctx.batch_detect_mixed_sets_dev(pcm.data_ptr(), 1, S, N, N, bank, rows.data_ptr(), SET, mbank, mrows.data_ptr(), SET, cfg, "f32", det.data_ptr(),
                                        det_ww.data_ptr(), det_label.data_ptr(), n_det.data_ptr(), MAX_DET)
        ctx.synchronize()

    def pair_of_calls():
        ctx.batch_detect_bank_sets_dev(pcm.data_ptr(), 1, S, N, N, bank, rows.data_ptr(), SET, cfg, det.data_ptr(), det_ww.data_ptr(), n_det.data_ptr(), MAX_DET)
        ctx.batch_detect_model_bank_sets_dev(pcm.data_ptr(), 1, S, N, N, mbank, mrows.data_ptr(), SET, cfg, "f32", det.data_ptr(), det_ww.data_ptr(),
                                             det_label.data_ptr(), n_det.data_ptr(), MAX_DET)
        ctx.synchronize()

    res = medians({"mixed": mixed_call, "pair": pair_of_calls}, 1)
    print(json.dumps(dict(common, metric="ms: one rp_batch_detect_mixed_sets call against rp_batch_detect_bank_sets + rp_batch_detect_model_bank_sets (whole recordings of 4 s)",
                          ms=res, mixed_over_pair=round(res["mixed"]["median_ms"] / res["pair"]["median_ms"], 3),
                          device=torch.cuda.get_device_name(0), build=ra.build_info())), flush=True)
else:
    CHUNKS = nums[1]
    N = CHUNKS * 480
    f32 = torch.empty((S, 4 * N), dtype=torch.float32, device="cuda")
    ctx.synth_dev(0x5EED, 0, S, 4 * N, 4 * N, f32.data_ptr())
    pcm = [to_i16(f32[:, j * N:(j + 1) * N]) for j in range(4)]   # a few calls' worth of different audio, reused round after round
    del f32
    one = ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=CHUNKS, bank=bank, stream_wakewords=int(rows.data_ptr()), set_size=SET,
                         model_bank=mbank, stream_models=int(mrows.data_ptr()), model_set_size=SET)
    pair = [ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=CHUNKS, bank=bank, stream_wakewords=int(rows.data_ptr()), set_size=SET),
            ra.StreamBatch(ctx, None, cfg, S, max_chunks_per_call=CHUNKS, model_bank=mbank, stream_models=int(mrows.data_ptr()), set_size=SET)]
    count = {"mixed": 0, "pair": 0}

    def calls(k, n):
        for _ in range(n):
            p = pcm[count[k] % 4].data_ptr()
            for sb in ([one] if k == "mixed" else pair):
                sb.process_dev(p, 1, CHUNKS, N, det.data_ptr(), n_det.data_ptr(), MAX_DET)
            count[k] += 1
        ctx.synchronize()

    # both sides past the point where every stream's window is full (195 frames) before anything is timed
    fill = (L + 3 * CHUNKS - 1) // (3 * CHUNKS) + 1
    for k in count:
        calls(k, fill)
    res = medians({k: (lambda k=k: calls(k, args.calls)) for k in count}, args.calls)
    print(json.dumps(dict(common, metric="ms per step of `chunks_per_call` chunks: one live-stream batch over mixed sets against one over wakeword sets plus one over model sets",
                          chunks_per_call=CHUNKS, calls_per_round=args.calls, ms=res,
                          mixed_over_pair=round(res["mixed"]["median_ms"] / res["pair"]["median_ms"], 3),
                          device=torch.cuda.get_device_name(0), build=ra.build_info())), flush=True)
