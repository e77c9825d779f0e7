#!/usr/bin/env python3
"""Raft and its FeatureEncoder: time per call against the same weights through the reference's composition
(encoder.py:15-55, model.py:66-97) in stock torch ops on the same device, in the same run.

    python scripts/bench_raft.py [--calls 30] [--warmup 5] [--out profiles/raft_bench.jsonl]

Two shapes: the reference's own (model.py:101-117: B 5, 60 x 60, 5 iterations, its widths, 3 levels of radius 3) and a 440 x 1024 pair
at RAFT's usual widths (feature 256, hidden and context 128, 4 levels of radius 4, 12 iterations).  Method as in bench_update_block.py:
every call timed on its own with a pair of events after a warm-up, median / p10 / p90 of `calls` calls; float32 on both sides.  The
torch side is written out here: conv2d / batch_norm (eval) / relu for the encoders, matmul / avg_pool2d / grid_sample for the
correlation pyramid, the update block's composition and the unfold-softmax upsampling, line by line as the reference has them.  One
JSON line per row (`row`: "feature_encoder" over the two stacked images, or "forward"):
  fused_ms, fused_ms_p10/p90          this package (FeatureEncoder: 17 launches; forward: 17 + 18 + 1 for the correlation build + iterations * 15)
  torch_ms, torch_ms_p10/p90          the torch composition
  fused_speedup_vs_torch              torch over fused
  max_abs_vs_torch                    largest |difference| (the two sum in different orders)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import feature_tracker_amd as F  # noqa: E402
from feature_tracker_amd import _native  # noqa: E402
from scripts.bench_scenes import RAFT_SHAPES as SHAPES  # noqa: E402
from scripts.benchlib import event_times, ms_fields, parser, write_rows  # noqa: E402
from tests.test_raft_encoder_cpu import make_image, make_raft_state, torch_encoder, torch_raft  # noqa: E402


def rows(args, torch):
    for name, widths, B, H, W, iterations in SHAPES:
        if name not in args.shapes.split(","):
            continue
        state = {k: v.to("cuda") for k, v in make_raft_state(widths, 1).items()}
        ref_image, cur_image = make_image(B, 1, H, W, 1).to("cuda"), make_image(B, 1, H, W, 2).to("cuda")
        model = F.Raft.from_state_dict(state, widths[3], widths[4], max_iterations=iterations)
        stacked = torch.cat([ref_image, cur_image], 0)
        normalised = 2.0 * (stacked / 255.0) - 1.0
        pairs = {
            "feature_encoder": (lambda: model.feature_encoder(stacked, normalise=True),
                                lambda: torch_encoder(state, normalised, "feature_encoder.", torch.float32)),
            "forward": (lambda: model(ref_image, cur_image)[-1],
                        lambda: torch_raft(state, ref_image, cur_image, widths[3], widths[4], iterations, torch.float32)[-1]),
        }
        with torch.no_grad():
            for row, (fused, stock) in pairs.items():
                f_ms = event_times(torch, [fused], args.calls, args.warmup)
                t_ms = event_times(torch, [stock], args.calls, args.warmup)
                line = dict(shape=name, row=row, B=B, H=H, W=W, iterations=iterations, widths=list(widths), calls=args.calls)
                ms_fields(line, "fused", f_ms, spread=True, digits=None)
                ms_fields(line, "torch", t_ms, spread=True, digits=None)
                line.update(fused_speedup_vs_torch=t_ms[0] / f_ms[0], max_abs_vs_torch=float((fused() - stock()).abs().max()))
                yield line


def main():
    ap = parser("--calls", 30, 5)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_raft.py needs a HIP device"
    write_rows(rows(args, torch), args.out, append=True, extra=dict(source_hash=_native.build_info().get("source_hash"), device=torch.cuda.get_device_name(0)))


if __name__ == "__main__":
    main()
