#!/usr/bin/env python3
"""SepConvGru (RAFT's separable ConvGRU): time per call against the same weights through the reference's
composition (gru.py:59-76) in stock torch ops on the same device, in the same run.

    python scripts/bench_sep_conv_gru.py [--calls 100] [--warmup 10] [--out profiles/sep_conv_gru_bench.jsonl]

Two shapes: the reference's model.py configuration (x 160, h 64 on the 8 x 8 grid its stride-8 encoder makes of the 60 x 60 example
images, batch 5 as model.py:101 has it), and RAFT's usual one (x 128 + 128, h 128, 1 x 55 x 128).  Method as in
bench_flow_upsample.py: every call timed on its own with a pair of events after a warm-up, median / p10 / p90 of `calls` calls; float32
on both sides.  One JSON line per shape:
  fused_ms, fused_ms_p10/p90          SepConvGru with x as ONE tensor
  fused_parts_ms                      SepConvGru with x as the parts a RAFT loop holds (no cat anywhere)
  torch_ms                            the torch composition given x as one tensor (its two cats per pass included, as in the reference)
  torch_parts_ms                      the same, with the cat of the parts in front of it (update_block.py:41,63)
  fused_speedup_vs_torch[_parts]      torch over fused
  max_abs_vs_torch                    largest |difference| of the two results (they differ in summation order)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import feature_tracker_amd as F  # noqa: E402
from feature_tracker_amd import _native  # noqa: E402
from tests.test_sep_conv_gru_cpu import make_state, torch_forward  # noqa: E402

# (name, the channels of the parts of x, h_channels, B, H, W)
SHAPES = [("model_py_60x60", (64, 96), 64, 5, 8, 8), ("raft_55x128", (128, 128), 128, 1, 55, 128)]


def time_gpu(torch, fn, calls, warmup):
    for _ in range(max(warmup, 1)):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.percentile(ms, 10)), float(np.percentile(ms, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    dev = torch.device("cuda")
    build = _native.build_info().get("source_hash", "?")
    rows = []
    for name, part_channels, Ch, B, H, W in SHAPES:
        Cx = sum(part_channels)
        state = {k: v.to(dev) for k, v in make_state(Cx, Ch, 5, 1).items()}
        gru = F.SepConvGru.from_state_dict(state)
        g = torch.Generator().manual_seed(Cx + H)
        parts = [torch.randn(B, c, H, W, generator=g).to(dev) for c in part_channels]
        h = torch.randn(B, Ch, H, W, generator=g).to(dev)
        x = torch.cat(parts, 1)
        with torch.no_grad():
            t = {
                "fused": time_gpu(torch, lambda: gru(x, h), args.calls, args.warmup),
                "fused_parts": time_gpu(torch, lambda: gru(parts, h), args.calls, args.warmup),
                "torch": time_gpu(torch, lambda: torch_forward(state, x, h), args.calls, args.warmup),
                "torch_parts": time_gpu(torch, lambda: torch_forward(state, torch.cat(parts, 1), h), args.calls, args.warmup),
            }
            diff = float((gru(parts, h) - torch_forward(state, x, h)).abs().max())
        row = {"shape": name, "x_parts": list(part_channels), "h_channels": Ch, "kernel_size": 5, "B": B, "H": H, "W": W}
        for key, (med, p10, p90) in t.items():
            row[key + "_ms"] = round(med, 4)
            if key == "fused":
                row["fused_ms_p10"], row["fused_ms_p90"] = round(p10, 4), round(p90, 4)
        row["fused_speedup_vs_torch"] = round(t["torch"][0] / t["fused"][0], 2)
        row["fused_speedup_vs_torch_parts"] = round(t["torch_parts"][0] / t["fused_parts"][0], 2)
        row["max_abs_vs_torch"] = diff
        row["flop"] = 2 * 2 * 3 * Ch * (Cx + Ch) * 5 * B * H * W
        row["fused_tflops"] = round(row["flop"] / (t["fused"][0] * 1e-3) / 1e12, 2)
        row["build"] = build
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
