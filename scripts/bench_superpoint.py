"""Time of SuperPoint.heads alone, at 480 x 752 and 480 x 640 with upstream's widths (64, 64, 128, 128, heads 256, D 256) and seeded random
weights, against the same weights through stock torch ops (``conv2d``, ``relu``, ``max_pool2d``, ``normalize``), and of ``conv1b`` with the
pool in its epilogue against ``conv2d_device`` followed by torch's ``max_pool2d``.  The torch composition is a
yardstick for time only: its convolutions sum in their own order.  Calls are interleaved in one process and the medians of
device-synchronised wall times over --repeats calls (default 30) are reported, one JSON line per shape (appended to --out, default
profiles/superpoint_bench.jsonl).  No time is asserted anywhere."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_scenes import WIDTHS, make_state  # noqa: E402
from scripts.benchlib import interleaved, parser, us_fields, write_rows  # noqa: E402

SHAPES = {"euroc_752x480": (480, 752), "vga_640x480": (480, 640)}
TRUNK = ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b")
POOLED = ("conv1b", "conv2b", "conv3b")


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


def rows(args, torch):
    import feature_tracker_amd as F
    from feature_tracker_amd import device as D
    from feature_tracker_amd.raft import _device_context

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
            times = interleaved(torch, calls, args.repeats, args.warmup)
            semi, desc = sp.heads(image)
            t_semi, t_desc = torch_heads(torch, state, image)
            row = {"bench": "superpoint", "shape": name, "height": H, "width": W, "widths": list(WIDTHS), "launches": F.superpoint.LAUNCHES,
                   "max_abs_semi_vs_torch": float((semi - t_semi).abs().max().item()), "max_abs_desc_vs_torch": float((desc - t_desc).abs().max().item()),
                   "conv1b_pool_equals_unfused": bool(torch.equal(pooled, unfused()))}
            for label in calls:
                us_fields(row, label, times[label])
            yield row


def main():
    args = parser("--repeats", 30, 5, os.path.join(ROOT, "profiles", "superpoint_bench.jsonl")).parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=True, extra={"device": torch.cuda.get_device_name(0)})


if __name__ == "__main__":
    main()
