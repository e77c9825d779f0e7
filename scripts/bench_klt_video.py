"""Per-frame time of KltVideoTracker against the same loop written with the public entries that existed before it:
host DetectGoodFeatures, a host filter of the new corners against the survivors, DeviceKlt.track, a read-back of status.  A translated
synthetic sequence at the reference's shape (752 x 480, 300 features, distance 25) and the headline's (640 x 480, 2 000 features,
distance 8); medians of the timed frames, one JSON line per shape (appended to --out when given)."""
from __future__ import annotations

import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_scenes import VIDEO_SHAPES as SHAPES  # noqa: E402
from scripts.bench_scenes import sequence  # noqa: E402
from scripts.benchlib import parser, us_median, wall_time, write_rows  # noqa: E402


def run_tracker(F, torch, images, n, distance, levels):
    flow = F.OpticalFlowBasicKlt()
    flow.options().kMaxTrackPointsNumber = n
    tracker = F.KltVideoTracker(flow, n, levels=levels, min_distance=distance)
    times = [wall_time(torch, lambda: tracker.track(image)) for image in images]
    return times, int(tracker.n_live.item())


def run_composition(F, torch, D, images_host, images, n, distance, levels):
    """The loop a caller had to write: everything it needs on the host comes back every frame."""
    stream = torch.cuda.Stream()
    ctx = D.context_on_stream(stream)
    options = F.OpticalFlowOptions()
    options.kMaxTrackPointsNumber = n
    det = F.FeaturePointHarrisDetector(ctx)
    det.options().kMinFeatureDistance = distance
    pyramids = [F.ImagePyramid.build(images_host[0], levels, ctx), F.ImagePyramid.build(images_host[0], levels, ctx)]
    points = np.zeros((0, 2), np.float32)
    times, spare = [], 0
    with torch.cuda.stream(stream):
        for k, image in enumerate(images):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cur, prev = pyramids[spare], pyramids[1 - spare]
            cur.update(int(image.data_ptr()), "device")
            if k > 0 and len(points):
                uv = torch.from_numpy(points).cuda()
                status = torch.zeros(len(points), dtype=torch.uint8, device="cuda")
                out = torch.empty_like(uv)
                D.DeviceKlt("basic", options, prev, cur, ctx).track(uv, uv, status, out, status)
                keep = status.cpu().numpy() == 1  # the read-back
                points = out.cpu().numpy()[keep]
            _, corners = det.DetectGoodFeatures(cur, n)
            if len(points) and len(corners):
                far = np.abs(corners[:, None, :] - np.floor(points[None, :, :] + 0.5)).max(axis=2).min(axis=1) >= distance
                corners = corners[far]
            points = np.concatenate([points, corners[:n - len(points)]]).astype(np.float32)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            spare = 1 - spare
    return times, len(points)


def rows(args, torch):
    import feature_tracker_amd as F
    from feature_tracker_amd import device as D

    for name, (width, height, n, distance) in SHAPES.items():
        host = sequence(width, height, args.frames + args.warmup)
        images = [torch.from_numpy(i).cuda() for i in host]
        t_new, live_new = run_tracker(F, torch, images, n, distance, args.levels)
        t_old, live_old = run_composition(F, torch, D, host, images, n, distance, args.levels)
        row = {"bench": "klt_video", "shape": name, "width": width, "height": height, "max_features": n, "min_distance": distance, "frames": args.frames,
               "tracker_us_median": us_median(t_new[args.warmup:]), "composition_us_median": us_median(t_old[args.warmup:]),
               "tracker_live": live_new, "composition_live": live_old, "device": torch.cuda.get_device_name(0)}
        row["speedup"] = round(row["composition_us_median"] / row["tracker_us_median"], 2)
        yield row


def main():
    ap = parser("--frames", 30, 5)
    ap.add_argument("--levels", type=int, default=4)
    args = ap.parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=True)


if __name__ == "__main__":
    main()
