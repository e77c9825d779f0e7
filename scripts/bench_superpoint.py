"""Time of SuperPoint.heads alone, at 480 x 752 and 480 x 640 with upstream's widths (64, 64, 128, 128, heads 256, D 256) and seeded random
weights, against the same weights through stock torch ops (``conv2d``, ``relu``, ``max_pool2d``, ``normalize``), and of ``conv1b`` with the
pool in its epilogue against ``conv2d_device`` followed by torch's ``max_pool2d``.  The torch composition is a
yardstick for time only: its convolutions sum in their own order.  Calls are interleaved in one process and the medians of
device-synchronised wall times over --repeats calls (default 30) are reported, one JSON line per shape (appended to --out, default
profiles/superpoint_bench.jsonl).  No time is asserted anywhere."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"euroc_752x480": (480, 752), "vga_640x480": (480, 640)}
WIDTHS = (64, 64, 128, 128, 256, 256)  # conv1, conv2, conv3, conv4, the heads' hidden layers, D
TRUNK = ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b")
POOLED = ("conv1b", "conv2b", "conv3b")


def make_state(torch, widths, seed):
    c1, c2, c3, c4, head, d = widths
    shapes = {"conv1a": (c1, 1, 3), "conv1b": (c1, c1, 3), "conv2a": (c2, c1, 3), "conv2b": (c2, c2, 3), "conv3a": (c3, c2, 3), "conv3b": (c3, c3, 3),
              "conv4a": (c4, c3, 3), "conv4b": (c4, c4, 3), "convPa": (head, c4, 3), "convPb": (65, head, 1), "convDa": (head, c4, 3), "convDb": (d, head, 1)}
    torch.manual_seed(seed)
    state = {}
    for name, (M, Cin, ks) in shapes.items():
        conv = torch.nn.Conv2d(Cin, M, ks, stride=1, padding=ks // 2)
        state[name + ".weight"], state[name + ".bias"] = conv.weight.detach().cuda(), conv.bias.detach().cuda()
    return state


def torch_heads(torch, state, image):
    F = torch.nn.functional
    conv = lambda x, name: F.conv2d(x, state[name + ".weight"], state[name + ".bias"], padding=state[name + ".weight"].shape[-1] // 2)  # noqa: E731
    x = image[None, None]
    for name in TRUNK:
        x = F.relu(conv(x, name))
        if name in POOLED:
            x = F.max_pool2d(x, 2, 2)
    semi = conv(F.relu(conv(x, "convPa")), "convPb")
    desc = F.normalize(conv(F.relu(conv(x, "convDa")), "convDb"), p=2, dim=1)
    return semi[0], desc[0]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "superpoint_bench.jsonl"))
    args = ap.parse_args()
    import torch

    import feature_tracker_amd as F
    from feature_tracker_amd import device as D
    from feature_tracker_amd.raft import _device_context

    rows = []
    with torch.no_grad():
        state = make_state(torch, WIDTHS, 1)
        sp = F.SuperPoint.from_state_dict(state)
        for name, (H, W) in SHAPES.items():
            image = torch.from_numpy(np.random.default_rng(1).uniform(0.0, 1.0, (H, W)).astype(np.float32)).cuda()
            ctx = _device_context(image)
            sp.heads(image)
            bufs = sp._buffers[(image.device, H, W)]
            x = bufs["conv1a"]
            weights, bias, ks, M = sp._layers["conv1b"]
            pooled, full = torch.empty_like(bufs["conv1b"]), torch.empty_like(x)

            def unfused():
                D.conv2d_device(ctx, [x], weights, bias, ks, True, 1.0, full)
                return torch.nn.functional.max_pool2d(full, 2, 2)

            calls = {"heads": lambda: sp.heads(image), "torch_ops": lambda: torch_heads(torch, state, image),
                     "conv1b_pool": lambda: D.conv2d_pool_device(ctx, [x], weights, bias, ks, True, pooled), "conv1b_then_torch_pool": unfused}
            times = {label: [] for label in calls}
            for _ in range(3):  # interleaved rounds
                for label, fn in calls.items():
                    times[label] += timed(torch, fn, args.repeats // 3, args.warmup)
            semi, desc = sp.heads(image)
            t_semi, t_desc = torch_heads(torch, state, image)
            row = {"bench": "superpoint", "shape": name, "height": H, "width": W, "widths": list(WIDTHS), "launches": F.superpoint.LAUNCHES,
                   "max_abs_semi_vs_torch": float((semi - t_semi).abs().max().item()), "max_abs_desc_vs_torch": float((desc - t_desc).abs().max().item()),
                   "conv1b_pool_equals_unfused": bool(torch.equal(pooled, unfused()))}
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
