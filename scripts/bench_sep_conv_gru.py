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
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import feature_tracker_amd as F  # noqa: E402
from feature_tracker_amd import _native  # noqa: E402
from scripts.benchlib import event_times, ms_fields, parser, write_rows  # noqa: E402
from tests.test_sep_conv_gru_cpu import make_state, torch_forward  # noqa: E402

# (name, the channels of the parts of x, h_channels, B, H, W)
SHAPES = [("model_py_60x60", (64, 96), 64, 5, 8, 8), ("raft_55x128", (128, 128), 128, 1, 55, 128)]


def rows(args, torch):
    dev = torch.device("cuda")
    for name, part_channels, Ch, B, H, W in SHAPES:
        Cx = sum(part_channels)
        state = {k: v.to(dev) for k, v in make_state(Cx, Ch, 5, 1).items()}
        gru = F.SepConvGru.from_state_dict(state)
        g = torch.Generator().manual_seed(Cx + H)
        parts = [torch.randn(B, c, H, W, generator=g).to(dev) for c in part_channels]
        h = torch.randn(B, Ch, H, W, generator=g).to(dev)
        x = torch.cat(parts, 1)
        calls = {"fused": lambda: gru(x, h), "fused_parts": lambda: gru(parts, h), "torch": lambda: torch_forward(state, x, h),
                 "torch_parts": lambda: torch_forward(state, torch.cat(parts, 1), h)}
        with torch.no_grad():
            t = {key: event_times(torch, [fn], args.calls, args.warmup) for key, fn in calls.items()}
            diff = float((gru(parts, h) - torch_forward(state, x, h)).abs().max())
        row = {"shape": name, "x_parts": list(part_channels), "h_channels": Ch, "kernel_size": 5, "B": B, "H": H, "W": W}
        for key in t:
            ms_fields(row, key, t[key], spread=key == "fused")
        row["fused_speedup_vs_torch"] = round(t["torch"][0] / t["fused"][0], 2)
        row["fused_speedup_vs_torch_parts"] = round(t["torch_parts"][0] / t["fused_parts"][0], 2)
        row["max_abs_vs_torch"] = diff
        row["flop"] = 2 * 2 * 3 * Ch * (Cx + Ch) * 5 * B * H * W
        row["fused_tflops"] = round(row["flop"] / (t["fused"][0] * 1e-3) / 1e12, 2)
        yield row


def main():
    args = parser("--calls", 100, 10).parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=False, extra={"build": _native.build_info().get("source_hash", "?")})


if __name__ == "__main__":
    main()
