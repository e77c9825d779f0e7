"""Time of TwoViewRansac.filter alone, at M = 300 and 2 000 participants with K = 512 and 2 048 hypotheses, in its three modes, with
EpipolarRansac.filter timed in the same run as the yardstick, and of a KltVideoTracker frame without a filter and with each
``epipolar_model``.  The scene is scripts/bench_epipolar.py's (30 % outliers); calls are interleaved in one
process and the medians of device-synchronised wall times are reported, one JSON line per configuration (appended to --out, default
profiles/two_view_bench.jsonl).  No time is asserted anywhere."""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_scenes import IMAGE, VIDEO_SHAPES, sequence, two_view_scene  # noqa: E402
from scripts.benchlib import interleaved, parser, us_fields, us_median, wall_time, write_rows  # noqa: E402

MODES = ("fundamental", "homography", "auto")


def rows(args, torch):
    import feature_tracker_amd as F

    for M in (300, 2000):
        ref, cur = two_view_scene(M)
        d_ref, d_cur = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda()
        fresh = torch.ones(M, dtype=torch.uint8, device="cuda")
        for K in (512, 2048):
            filters = {"epipolar": F.EpipolarRansac(hypotheses=K, threshold=1.0, seed=1)}
            filters.update({mode: F.TwoViewRansac(model=mode, hypotheses=K, threshold=1.0, seed=1) for mode in MODES})
            status = {name: fresh.clone() for name in filters}

            def call(name):
                status[name].copy_(fresh)
                return filters[name].filter(d_ref, d_cur, status[name], IMAGE)

            times = interleaved(torch, {name: (lambda name=name: call(name)) for name in filters}, args.repeats, args.warmup)
            row = {"bench": "two_view_filter", "participants": M, "hypotheses": K}
            for name in filters:
                us_fields(row, name, times[name])
                row[f"{name}_kept"] = int((status[name] == 1).sum().item())
            yield row
    for name, (width, height, n, distance) in VIDEO_SHAPES.items():
        images = [torch.from_numpy(i).cuda() for i in sequence(width, height, args.frames + args.warmup)]
        row = {"bench": "klt_video_two_view", "shape": name, "width": width, "height": height, "max_features": n, "hypotheses": 512}
        for label, kw in [("plain", {})] + [(mode, {"epipolar_threshold": 1.0, "epipolar_hypotheses": 512, "epipolar_model": mode}) for mode in MODES]:
            flow = F.OpticalFlowBasicKlt()
            flow.options().kMaxTrackPointsNumber = n
            tracker = F.KltVideoTracker(flow, n, levels=4, min_distance=distance, **kw)
            times = [wall_time(torch, lambda: tracker.track(image)) for image in images]
            row[f"frame_{label}_us_median"] = us_median(times[args.warmup:])
            row[f"live_{label}"] = int(tracker.n_live.item())
        yield row


def main():
    ap = parser("--repeats", 30, 5, os.path.join(ROOT, "profiles", "two_view_bench.jsonl"))
    ap.add_argument("--frames", type=int, default=30)
    args = ap.parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=True, extra={"device": torch.cuda.get_device_name(0)})


if __name__ == "__main__":
    main()
