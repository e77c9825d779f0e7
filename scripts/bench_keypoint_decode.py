"""Time of KeypointDecoder.decode alone, at 480 x 752 with K = 300 and D = 256 and at 480 x 640 with K = 2 000, in both descriptor layouts,
against the same five steps in stock torch ops.  The torch composition is ``softmax``, ``pixel_shuffle``,
``max_pool2d`` suppression, ``topk``, ``grid_sample`` and ``normalize``; it is a different algorithm in three places and is a yardstick for
time only: a pixel survives there iff it equals its window's maximum score (equal scores all survive, no pixel index breaks the tie), there
are no occupied points, ``topk`` needs K candidates (the rows behind the count are not zeros), and ``grid_sample`` evaluates the bilinear
blend in its own order.  Calls are interleaved in one process and the medians of device-synchronised wall times are reported, one JSON line
per shape (appended to --out, default profiles/keypoint_decode_bench.jsonl).  No time is asserted anywhere."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.benchlib import interleaved, parser, us_fields, write_rows  # noqa: E402

SHAPES = {"euroc_752x480": (480, 752, 300, 256, 20), "vga_640x480": (480, 640, 2000, 256, 4)}  # H, W, K, D, min_distance


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


def rows(args, torch):
    import feature_tracker_amd as F

    for name, (H, W, K, D, distance) in SHAPES.items():
        hc, wc = H // 8, W // 8
        rng = np.random.default_rng(1)
        semi = torch.from_numpy((2.5 * rng.standard_normal((65, hc, wc))).astype(np.float32)).cuda()
        desc = torch.from_numpy(rng.standard_normal((D, hc, wc)).astype(np.float32)).cuda()
        desc_last = desc.permute(1, 2, 0).contiguous().permute(2, 0, 1)
        decoder = F.KeypointDecoder(max_keypoints=K, min_score=0.05, min_distance=distance, border=4)
        calls = {"chw": lambda: decoder.decode(semi, desc), "hwc": lambda: decoder.decode(semi, desc_last),
                 "torch_ops": lambda: torch_composition(torch, semi, desc, K, 0.05, distance, 4)}
        times = interleaved(torch, calls, args.repeats, args.warmup)
        row = {"bench": "keypoint_decode", "shape": name, "height": H, "width": W, "max_keypoints": K, "channels": D, "min_distance": distance,
               "count": int(decoder.decode(semi, desc).count.item())}
        for label in calls:
            us_fields(row, label, times[label])
        yield row


def main():
    args = parser("--repeats", 30, 5, os.path.join(ROOT, "profiles", "keypoint_decode_bench.jsonl")).parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=True, extra={"device": torch.cuda.get_device_name(0)})


if __name__ == "__main__":
    main()
