"""Time of TwoViewRansac.filter alone, at M = 300 and 2 000 participants with K = 512 and 2 048 hypotheses, in its three modes, with
EpipolarRansac.filter timed in the same run as the yardstick, and of a KltVideoTracker frame without a filter and with each
``epipolar_model``.  The scene is scripts/bench_epipolar.py's (30 % outliers); calls are interleaved in one
process and the medians of device-synchronised wall times are reported, one JSON line per configuration (appended to --out, default
profiles/two_view_bench.jsonl).  No time is asserted anywhere."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("fundamental", "homography", "auto")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_bench.jsonl"))
    args = ap.parse_args()
    import torch

    import feature_tracker_amd as F
    from scripts.bench_epipolar import IMAGE, scene, timed
    from scripts.bench_klt_video import SHAPES, sequence

    rows = []
    for M in (300, 2000):
        ref, cur = scene(M)
        d_ref, d_cur = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda()
        fresh = torch.ones(M, dtype=torch.uint8, device="cuda")
        for K in (512, 2048):
            filters = {"epipolar": F.EpipolarRansac(hypotheses=K, threshold=1.0, seed=1)}
            filters.update({mode: F.TwoViewRansac(model=mode, hypotheses=K, threshold=1.0, seed=1) for mode in MODES})
            status = {name: fresh.clone() for name in filters}
            times = {name: [] for name in filters}

            def call(name):
                status[name].copy_(fresh)
                return filters[name].filter(d_ref, d_cur, status[name], IMAGE)

            for _ in range(3):  # interleaved rounds
                for name in filters:
                    times[name] += timed(torch, lambda: call(name), args.repeats // 3, args.warmup)
            row = {"bench": "two_view_filter", "participants": M, "hypotheses": K}
            for name in filters:
                row[f"{name}_us_median"] = round(1e6 * float(np.median(times[name])), 1)
                row[f"{name}_us_min"] = round(1e6 * float(np.min(times[name])), 1)
                row[f"{name}_kept"] = int((status[name] == 1).sum().item())
            rows.append(row)
    for name, (width, height, n, distance) in SHAPES.items():
        images = [torch.from_numpy(i).cuda() for i in sequence(width, height, args.frames + args.warmup)]
        row = {"bench": "klt_video_two_view", "shape": name, "width": width, "height": height, "max_features": n, "hypotheses": 512}
        for label, kw in [("plain", {})] + [(mode, {"epipolar_threshold": 1.0, "epipolar_hypotheses": 512, "epipolar_model": mode}) for mode in MODES]:
            flow = F.OpticalFlowBasicKlt()
            flow.options().kMaxTrackPointsNumber = n
            tracker = F.KltVideoTracker(flow, n, levels=4, min_distance=distance, **kw)
            times = []
            for image in images:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tracker.track(image)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            row[f"frame_{label}_us_median"] = round(1e6 * float(np.median(times[args.warmup:])), 1)
            row[f"live_{label}"] = int(tracker.n_live.item())
        rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for row in rows:
        row["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(row)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
