"""Time of KeypointDecoder.decode alone, at 480 x 752 with K = 300 and D = 256 and at 480 x 640 with K = 2 000, in both descriptor layouts,
against the same five steps in stock torch ops.  The torch composition is ``softmax``, ``pixel_shuffle``,
``max_pool2d`` suppression, ``topk``, ``grid_sample`` and ``normalize``; it is a different algorithm in three places and is a yardstick for
time only: a pixel survives there iff it equals its window's maximum score (equal scores all survive, no pixel index breaks the tie), there
are no occupied points, ``topk`` needs K candidates (the rows behind the count are not zeros), and ``grid_sample`` evaluates the bilinear
blend in its own order.  Calls are interleaved in one process and the medians of device-synchronised wall times are reported, one JSON line
per shape (appended to --out, default profiles/keypoint_decode_bench.jsonl).  No time is asserted anywhere."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"euroc_752x480": (480, 752, 300, 256, 20), "vga_640x480": (480, 640, 2000, 256, 4)}  # H, W, K, D, min_distance


def timed(torch, fn, repeats, warmup):
    out = []
    for i in range(repeats + warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(time.perf_counter() - t0)
    return out


def torch_composition(torch, semi, desc, K, min_score, min_distance, border):
    F = torch.nn.functional
    hc, wc = semi.shape[1:]
    prob = F.softmax(semi, dim=0)[:64]
    heat = F.pixel_shuffle(prob.reshape(1, 64, hc, wc), 8)[0, 0]
    peak = F.max_pool2d(heat[None, None], 2 * min_distance - 1, 1, min_distance - 1)[0, 0]
    keep = (heat == peak) & (heat > min_score)
    keep[:border], keep[-border:], keep[:, :border], keep[:, -border:] = False, False, False, False
    scores, idx = torch.topk(torch.where(keep, heat, torch.zeros_like(heat)).reshape(-1), K)
    W = heat.shape[1]
    uv = torch.stack([idx % W, idx // W], dim=1).float()
    grid = torch.stack([(uv[:, 0] - 3.5) / 8.0 / max(wc - 1, 1) * 2 - 1, (uv[:, 1] - 3.5) / 8.0 / max(hc - 1, 1) * 2 - 1], dim=1)
    sampled = F.grid_sample(desc[None], grid[None, None], mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0].t()
    return uv, scores, F.normalize(sampled, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypoint_decode_bench.jsonl"))
    args = ap.parse_args()
    import torch

    import feature_tracker_amd as F

    rows = []
    for name, (H, W, K, D, distance) in SHAPES.items():
        hc, wc = H // 8, W // 8
        rng = np.random.default_rng(1)
        semi = torch.from_numpy((2.5 * rng.standard_normal((65, hc, wc))).astype(np.float32)).cuda()
        desc = torch.from_numpy(rng.standard_normal((D, hc, wc)).astype(np.float32)).cuda()
        desc_last = desc.permute(1, 2, 0).contiguous().permute(2, 0, 1)
        decoder = F.KeypointDecoder(max_keypoints=K, min_score=0.05, min_distance=distance, border=4)
        calls = {"chw": lambda: decoder.decode(semi, desc), "hwc": lambda: decoder.decode(semi, desc_last),
                 "torch_ops": lambda: torch_composition(torch, semi, desc, K, 0.05, distance, 4)}
        times = {label: [] for label in calls}
        for _ in range(3):  # interleaved rounds
            for label, fn in calls.items():
                times[label] += timed(torch, fn, args.repeats // 3, args.warmup)
        row = {"bench": "keypoint_decode", "shape": name, "height": H, "width": W, "max_keypoints": K, "channels": D, "min_distance": distance,
               "count": int(decoder.decode(semi, desc).count.item())}
        for label in calls:
            row[f"{label}_us_median"] = round(1e6 * float(np.median(times[label])), 1)
            row[f"{label}_us_min"] = round(1e6 * float(np.min(times[label])), 1)
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
