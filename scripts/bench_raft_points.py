#!/usr/bin/env python3
"""Raft.track_points: time per call against what a caller composed before it existed, on the same weights,
images and points, in the same run.

    python scripts/bench_raft_points.py [--calls 30] [--warmup 5] [--out profiles/raft_points_bench.jsonl]

The two shapes of bench_raft.py, each with 300 and 2 000 points per image.  Method as there: every call timed on its own
with a pair of events after a warm-up, median / p10 / p90 of `calls` calls; float32.  One JSON line per (shape, points, row):
  track_points             Raft.track_points                              against  Raft.__call__, then grid_sample (align_corners=True) on the last
                                                                                   prediction and the bounds tests in torch
  track_points_fb          Raft.track_points(forward_backward=1.0)        against  two __call__s with swapped images, then the same composition twice
                                                                                   and the distance test
  kernel                   track_points_from_flow alone                   against  upsample_flow, then grid_sample and the bounds tests
with new_ms, old_ms (and their p10 / p90), old_over_new, and max_abs_points: the largest distance between the two routes' tracked
points (grid_sample's interpolation arithmetic is torch's own).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import feature_tracker_amd as F  # noqa: E402
from feature_tracker_amd import _native  # noqa: E402
from scripts.bench_scenes import RAFT_SHAPES as SHAPES  # noqa: E402
from scripts.benchlib import event_times, ms_fields, parser, write_rows  # noqa: E402
from tests.test_raft_encoder_cpu import make_image, make_raft_state  # noqa: E402

POINT_COUNTS = (300, 2000)


def torch_sample(torch, dense, points, H, W):
    """What a caller wrote: the dense flow sampled bilinearly at the points, the points moved, and the two bounds tests."""
    H8, W8 = dense.shape[2:]
    grid = torch.stack([2.0 * points[..., 0] / (W8 - 1) - 1.0, 2.0 * points[..., 1] / (H8 - 1) - 1.0], -1)[:, :, None]
    flow = torch.nn.functional.grid_sample(dense, grid, mode="bilinear", padding_mode="border", align_corners=True)[:, :, :, 0].permute(0, 2, 1)
    cur = points + flow

    def inside(p):
        return (p[..., 0] >= 0) & (p[..., 0] <= W - 1) & (p[..., 1] >= 0) & (p[..., 1] <= H - 1)

    return cur, inside(points) & inside(cur) & torch.isfinite(cur).all(-1)


def rows(args, torch):
    for name, widths, B, H, W, iterations in SHAPES:
        if name not in args.shapes.split(","):
            continue
        state = {k: v.to("cuda") for k, v in make_raft_state(widths, 1).items()}
        ref_image, cur_image = make_image(B, 1, H, W, 1).to("cuda"), make_image(B, 1, H, W, 2).to("cuda")
        model = F.Raft.from_state_dict(state, widths[3], widths[4], max_iterations=iterations)
        h, w = ((((e + 1) // 2 + 1) // 2 + 1) // 2 for e in (H, W))
        g = torch.Generator().manual_seed(7)
        flow, mask = (0.5 * torch.randn(B, 2, h, w, generator=g)).to("cuda"), torch.randn(B, 576, h, w, generator=g).to("cuda")
        for count in POINT_COUNTS:
            points = (torch.rand(B, count, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])).to("cuda")

            def old_fb():
                cur, ok = torch_sample(torch, model(ref_image, cur_image)[-1], points, H, W)
                back, ok_back = torch_sample(torch, model(cur_image, ref_image)[-1], cur.clamp(min=0).minimum(points.new_tensor([W - 1.0, H - 1.0])), H, W)
                return cur, ok & (((back - points) ** 2).sum(-1) <= 1.0)

            pairs = {
                "track_points": (lambda: model.track_points(ref_image, cur_image, points), lambda: torch_sample(torch, model(ref_image, cur_image)[-1], points, H, W)),
                "track_points_fb": (lambda: model.track_points(ref_image, cur_image, points, forward_backward=1.0), old_fb),
                "kernel": (lambda: F.track_points_from_flow(flow, mask, points, (H, W)), lambda: torch_sample(torch, F.upsample_flow(flow, mask), points, H, W)),
            }
            with torch.no_grad():
                for row, (new, old) in pairs.items():
                    n_ms = event_times(torch, [new], args.calls, args.warmup)
                    o_ms = event_times(torch, [old], args.calls, args.warmup)
                    got, want = new(), old()
                    both = (got[1] == F.TRACKED) & want[1]
                    line = dict(shape=name, row=row, points=count, B=B, H=H, W=W, iterations=iterations, widths=list(widths), calls=args.calls)
                    ms_fields(line, "new", n_ms, spread=True, digits=None)
                    ms_fields(line, "old", o_ms, spread=True, digits=None)
                    line.update(old_over_new=o_ms[0] / n_ms[0], tracked=int((got[1] == F.TRACKED).sum()),
                                max_abs_points=float((got[0] - want[0])[both].abs().max()) if bool(both.any()) else None)
                    yield line


def main():
    ap = parser("--calls", 30, 5)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_raft_points.py needs a HIP device"
    write_rows(rows(args, torch), args.out, append=True, extra=dict(source_hash=_native.build_info().get("source_hash"), device=torch.cuda.get_device_name(0)))


if __name__ == "__main__":
    main()
