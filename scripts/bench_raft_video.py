#!/usr/bin/env python3
"""RaftVideoTracker and warm_start_flow: time per frame against pairwise Raft.track_points on the same weights,
images and points, and the warm start alone against upstream RAFT's route through the host, in the same run.

    python scripts/bench_raft_video.py [--calls 30] [--warmup 5] [--out profiles/raft_video_bench.jsonl]

The two shapes of bench_raft.py, 300 points per image, a ring of four seeded frames.  Method as there: every call timed
on its own with a pair of events after a warm-up, median / p10 / p90 of `calls` calls; float32.  One JSON line per row:
  pairwise, pairwise_fb      Raft.track_points on consecutive frames of the ring, without and with forward_backward=1.0 (this tree's)
  video_cold                 RaftVideoTracker(warm_start=False).track: the cached feature map alone
  video_warm, video_warm_fb  RaftVideoTracker().track, without and with the check
  warm_start                 warm_start_flow alone at 8 x 8, 55 x 128 and 135 x 240, B 1 and 5, on a Gaussian flow (sigma 2): the automatic
                             form (`splits`, `launches`), the one-launch form forced, and upstream's forward_interpolate per entry with the
                             copies to the host and back (host_ms; null without scipy)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import feature_tracker_amd as F  # noqa: E402
from feature_tracker_amd import _native  # noqa: E402
from feature_tracker_amd import device as D  # noqa: E402
from feature_tracker_amd import raft as R  # noqa: E402
from scripts.bench_scenes import RAFT_SHAPES as SHAPES  # noqa: E402
from scripts.benchlib import event_times, ms_fields, parser, write_rows  # noqa: E402
from tests.test_raft_encoder_cpu import make_image, make_raft_state  # noqa: E402

POINTS = 300
WARM_SHAPES = [(8, 8), (55, 128), (135, 240)]
WARM_BATCHES = (1, 5)


def forward_interpolate(flow):
    """Upstream RAFT's forward_interpolate (core/utils/utils.py) on one [2, H, W] array."""
    from scipy import interpolate

    dx, dy = flow[0], flow[1]
    ht, wd = dx.shape
    x0, y0 = np.meshgrid(np.arange(wd), np.arange(ht))
    x1, y1 = (x0 + dx).reshape(-1), (y0 + dy).reshape(-1)
    dx, dy = dx.reshape(-1), dy.reshape(-1)
    valid = (x1 > 0) & (x1 < wd) & (y1 > 0) & (y1 < ht)
    x1, y1, dx, dy = x1[valid], y1[valid], dx[valid], dy[valid]
    flow_x = interpolate.griddata((x1, y1), dx, (x0, y0), method="nearest", fill_value=0)
    flow_y = interpolate.griddata((x1, y1), dy, (x0, y0), method="nearest", fill_value=0)
    return np.stack([flow_x, flow_y], axis=0).astype(np.float32)


def rows(args, torch):
    for name, widths, B, H, W, iterations in SHAPES:
        if name not in args.shapes.split(","):
            continue
        state = {k: v.to("cuda") for k, v in make_raft_state(widths, 1).items()}
        ring = [make_image(B, 1, H, W, 1 + k).to("cuda") for k in range(4)]
        model = F.Raft.from_state_dict(state, widths[3], widths[4], max_iterations=iterations)
        g = torch.Generator().manual_seed(7)
        points = (torch.rand(B, POINTS, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])).to("cuda")
        turn = [0]

        def pairwise(fb=None):
            turn[0] += 1
            return model.track_points(ring[(turn[0] - 1) % 4], ring[turn[0] % 4], points, forward_backward=fb)

        def video(tracker):
            def step():
                turn[0] += 1
                return tracker.track(ring[turn[0] % 4], points)
            return step

        trackers = {"video_cold": F.RaftVideoTracker(model, warm_start=False), "video_warm": F.RaftVideoTracker(model),
                    "video_warm_fb": F.RaftVideoTracker(model, forward_backward=1.0)}
        steps = {"pairwise": lambda: pairwise(), "pairwise_fb": lambda: pairwise(1.0)}
        with torch.no_grad():
            for row, tracker in trackers.items():
                tracker.track(ring[0])
                steps[row] = video(tracker)
            # two passes, alternating the rows, so that a drift of the machine falls on all of them
            timed = {row: [] for row in steps}
            for _ in range(2):
                for row, fn in steps.items():
                    timed[row].append(event_times(torch, [fn], args.calls, args.warmup))
        for row, passes in timed.items():
            ms = min(passes)
            line = dict(shape=name, row=row, points=POINTS, B=B, H=H, W=W, iterations=iterations, widths=list(widths), ms=ms[0], ms_p10=ms[1], ms_p90=ms[2],
                        ms_passes=[p[0] for p in passes], over_pairwise=ms[0] / min(timed["pairwise_fb" if row.endswith("_fb") else "pairwise"])[0])
            yield line

    if not args.no_warm_start_rows:
        try:
            import scipy  # noqa: F401
            have_scipy = True
        except ImportError:
            have_scipy = False
        for H, W in WARM_SHAPES:
            for B in WARM_BATCHES:
                flow = (2.0 * torch.randn(B, 2, H, W, generator=torch.Generator().manual_seed(H + B))).to("cuda")
                ctx = R._device_context(flow)
                splits = _native.flow_warm_splits(B, H, W)
                out = torch.empty_like(flow)

                def host():
                    f = flow.cpu().numpy()
                    return torch.from_numpy(np.stack([forward_interpolate(f[b]) for b in range(B)])).to("cuda")

                with torch.no_grad():
                    auto = event_times(torch, [lambda: F.warm_start_flow(flow)], args.calls, args.warmup)
                    one = event_times(torch, [lambda: D.flow_warm_device(ctx, flow, out, 1)], args.calls, args.warmup)
                    host_ms = event_times(torch, [host], args.calls, 1) if have_scipy else None
                    same = bool(torch.equal(F.warm_start_flow(flow), host())) if have_scipy else None
                line = dict(row="warm_start", B=B, H=H, W=W, splits=splits, launches=1 if splits == 1 else 2, ms=auto[0], ms_p10=auto[1], ms_p90=auto[2])
                ms_fields(line, "one_launch", one, spread=True, digits=None)
                line.update(host_ms=None if host_ms is None else host_ms[0], host_over_device=None if host_ms is None else host_ms[0] / auto[0], equal_to_host=same)
                yield line


def main():
    ap = parser("--calls", 30, 5)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--no-warm-start-rows", action="store_true")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_raft_video.py needs a HIP device"
    common = dict(calls=args.calls, source_hash=_native.build_info().get("source_hash"), device=torch.cuda.get_device_name(0))
    write_rows(rows(args, torch), args.out, append=True, extra=common)


if __name__ == "__main__":
    main()
