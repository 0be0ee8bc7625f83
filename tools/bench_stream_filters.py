"""What the filters cost a live-stream batch (rp_stream_batch_set_filters): one call of S streams x n chunks with filters off / band-pass
only / gain normaliser + band-pass, next to rp_frontend_batch (both filters, the stateless three-launch call) on the same S x 480 n samples.
All variants of a shape run in ONE process, warm, alternating, `--repeats` windows of `--calls` calls each ending in a device synchronise;
per variant the median window and the spread (min .. max) in ms per call.  One JSON line per shape; --out DIR also writes them to
DIR/bench_stream_filters_<n>chunks_<fmt>.json.
usage: python tools/bench_stream_filters.py [--streams 65536] [--chunks 1,8] [--fmts i16,f32] [--calls 50] [--repeats 7] [--out profiles]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import rustpotter_amd as ra

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=65536)
ap.add_argument("--chunks", default="1,8")
ap.add_argument("--fmts", default="i16,f32")
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--templates", type=int, default=8)
ap.add_argument("--template-len", type=int, default=100)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs a GPU"

S, L = args.streams, args.template_len
ctx = ra.BatchContext(0, host_pointers=False)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
lib = ra.load_library()
rng = np.random.default_rng(1)
tm = ra.Templates(ctx, [rng.standard_normal((L, 5)).astype(np.float32) for _ in range(args.templates)])
cfg = ra.DetectorConfig()
cfg.avg_threshold = 0.0


def filters(gain, band):
    f = ra.FiltersConfig()
    f.gain_normalizer.enabled, f.gain_normalizer.min_gain, f.gain_normalizer.max_gain = gain, 0.2, 3.0
    f.band_pass.enabled, f.band_pass.low_cutoff, f.band_pass.high_cutoff = band, 120.0, 900.0
    return f


for n in [int(x) for x in args.chunks.split(",")]:
    for fmt in args.fmts.split(","):
        N = 480 * n
        # four calls' worth of noise whose loudness differs from stream to stream (the gains are not all alike), cycled
        amp = torch.exp(torch.empty((S, 1), device="cuda").uniform_(np.log(0.01), np.log(0.6)))
        x = (torch.randn((S, 4 * N), device="cuda") * amp).clamp_(-1.0, 1.0)
        pcm, code = ((x * 32767.0).round().to(torch.int16), 1) if fmt == "i16" else (x, 3)
        width = pcm.element_size()
        det = torch.zeros((S, 4, 6), dtype=torch.int32, device="cuda")
        n_det = torch.zeros((S,), dtype=torch.int32, device="cuda")
        out = torch.empty((S, N), dtype=torch.float32, device="cuda")
        rc = ra.RustpotterConfig()
        rc.filters = filters(True, True)
        fc = rc._filters_c()
        calls = [0]

        def live(sb):
            def step():
                off = (calls[0] % 4) * N
                calls[0] += 1
                sb.process_dev(pcm.data_ptr() + width * off, code, n, pcm.shape[1], det.data_ptr(), n_det.data_ptr(), 4)
            return step

        def frontend():
            off = (calls[0] % 4) * N
            calls[0] += 1
            assert lib.rp_frontend_batch(ctx._h, pcm.data_ptr() + width * off, code, S, N, pcm.shape[1], C.byref(fc), 0.05, L // 3,
                                         out.data_ptr(), N, None, None) == 0

        variants = {
            "live_off": live(ra.StreamBatch(ctx, tm, cfg, S, max_chunks_per_call=n)),
            "live_band_pass": live(ra.StreamBatch(ctx, tm, cfg, S, max_chunks_per_call=n, filters=filters(False, True))),
            "live_gain_band_pass": live(ra.StreamBatch(ctx, tm, cfg, S, max_chunks_per_call=n, filters=filters(True, True), rms_level_ref=0.05)),
            "frontend_batch": frontend,
        }
        for step in variants.values():   # fill the windows: every timed call scores complete windows
            for _ in range(-(-L // (3 * n)) + 4):
                step()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, step in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    step()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / args.calls * 1e3)
        res = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms.items()}
        extra = res["live_gain_band_pass"]["median_ms"] - res["live_off"]["median_ms"]
        line = {"metric": "ms per live call, filters off / on, next to rp_frontend_batch on the same samples", "streams": S, "chunks_per_call": n,
                "input": fmt, "templates": "%d x %d frames" % (args.templates, L), "calls_per_window": args.calls, "windows": args.repeats,
                "ms_per_call": res, "filters_extra_ms": round(extra, 4),
                "band_pass_extra_ms": round(res["live_band_pass"]["median_ms"] - res["live_off"]["median_ms"], 4),
                "frontend_batch_ms": res["frontend_batch"]["median_ms"], "device": torch.cuda.get_device_name(0), "build": ra.build_info()}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(os.path.join(args.out, "bench_stream_filters_%dchunks_%s.json" % (n, fmt)), "w") as fh:
                fh.write(text + "\n")
