"""Time of EpipolarRansac.filter alone, at M = 300 and 2 000 participants with K = 512 and 2 048 hypotheses, against the same contract written
in stock torch ops on the device (the sampler's integer mix, a batched null vector by torch.linalg.svd in place of the elimination, the
Sampson test as one [K, M] tensor expression, argmax, the status rewrite), and of a KltVideoTracker frame with and without the filter
(DESIGN.md 5.20 and 6).  Both sides run on a synthetic two-view scene with 30 % outliers; calls are interleaved in one process and the
medians of device-synchronised wall times are reported, one JSON line per configuration (appended to --out when given)."""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_scenes import IMAGE, VIDEO_SHAPES, sequence, two_view_scene  # noqa: E402
from scripts.benchlib import interleaved, parser, us_fields, us_median, wall_time, write_rows  # noqa: E402


def torch_filter(torch, ref_uv, cur_uv, status, image, threshold, K, seed):
    """The contract in stock torch ops: everything on the device, nothing read back."""
    H, W = image
    dev = ref_uv.device
    cx, cy, s = 0.5 * (W - 1), 0.5 * (H - 1), 2.0 / (W + H)
    part = torch.nonzero(status == 1).squeeze(1)
    M = part.numel()  # (a host read: boolean indexing has no fixed-shape form in stock ops)
    centre = torch.tensor([cx, cy], device=dev)
    x1, x2 = (ref_uv[part] - centre) * s, (cur_uv[part] - centre) * s
    mask = 0xFFFFFFFF

    def fmix(x):
        x = x ^ (x >> 16)
        x = (x * 0x85EBCA6B) & mask
        x = x ^ (x >> 13)
        x = (x * 0xC2B2AE35) & mask
        return x ^ (x >> 16)

    h = torch.arange(K, device=dev, dtype=torch.int64)[:, None, None]
    ka = (torch.arange(8, device=dev, dtype=torch.int64)[None, :, None] * 16 + torch.arange(16, device=dev, dtype=torch.int64)[None, None, :] + 1)
    draws = (fmix(fmix((seed + 0x9E3779B9 * (h + 1)) & mask) ^ ((0x85EBCA6B * ka) & mask)) * M) >> 32  # [K, 8, 16]
    idx = torch.zeros((K, 8), dtype=torch.int64, device=dev)
    ok = torch.ones(K, dtype=torch.bool, device=dev)
    for k in range(8):
        fresh = (draws[:, k, :, None] != idx[:, None, :k]).all(dim=2)  # [K, 16]
        first = fresh.int().argmax(dim=1)
        ok &= fresh.any(dim=1)
        idx[:, k] = draws[:, k].gather(1, first[:, None]).squeeze(1)
    a1, a2 = x1[idx], x2[idx]  # [K, 8, 2]
    A = torch.stack([a2[..., 0] * a1[..., 0], a2[..., 0] * a1[..., 1], a2[..., 0], a2[..., 1] * a1[..., 0], a2[..., 1] * a1[..., 1], a2[..., 1],
                     a1[..., 0], a1[..., 1], torch.ones_like(a1[..., 0])], dim=2)
    F = torch.linalg.svd(A, full_matrices=True).Vh[:, 8, :].reshape(K, 3, 3)
    p1 = torch.cat([x1, torch.ones(M, 1, device=dev)], dim=1)
    p2 = torch.cat([x2, torch.ones(M, 1, device=dev)], dim=1)
    a = torch.einsum("kij,mj->kmi", F, p1)
    b = torch.einsum("kji,mj->kmi", F, p2)
    num = (a * p2[None]).sum(dim=2)
    den = a[..., 0] ** 2 + a[..., 1] ** 2 + b[..., 0] ** 2 + b[..., 1] ** 2
    inl = (num * num <= (threshold * s) ** 2 * den) & (den > 0)
    counts = torch.where(ok, inl.sum(dim=1), torch.full_like(ok, -1, dtype=torch.int64))
    best = counts.argmax()
    rejected = part[~inl[best]]
    status[rejected] = 2
    return best, counts[best]


def rows(args, torch):
    import feature_tracker_amd as F

    for M in (300, 2000):
        ref, cur = two_view_scene(M)
        d_ref, d_cur = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda()
        fresh = torch.ones(M, dtype=torch.uint8, device="cuda")
        for K in (512, 2048):
            ransac = F.EpipolarRansac(hypotheses=K, threshold=1.0, seed=1)
            status_a, status_b = fresh.clone(), fresh.clone()

            def ours():
                status_a.copy_(fresh)
                return ransac.filter(d_ref, d_cur, status_a, IMAGE)

            def stock():
                status_b.copy_(fresh)
                return torch_filter(torch, d_ref, d_cur, status_b, IMAGE, 1.0, K, 1)

            times = interleaved(torch, {"filter": ours, "torch_ops": stock}, args.repeats, args.warmup)
            row = {"bench": "epipolar_filter", "participants": M, "hypotheses": K}
            for name in times:
                us_fields(row, name, times[name])
            row["kept"], row["torch_ops_kept"] = int((status_a == 1).sum().item()), int((status_b == 1).sum().item())
            yield row
    for name, (width, height, n, distance) in VIDEO_SHAPES.items():
        images = [torch.from_numpy(i).cuda() for i in sequence(width, height, args.frames + args.warmup)]
        medians = {}
        for label, kw in (("plain", {}), ("filtered", {"epipolar_threshold": 1.0, "epipolar_hypotheses": 512})):
            flow = F.OpticalFlowBasicKlt()
            flow.options().kMaxTrackPointsNumber = n
            tracker = F.KltVideoTracker(flow, n, levels=4, min_distance=distance, **kw)
            times = [wall_time(torch, lambda: tracker.track(image)) for image in images]
            medians[label] = (us_median(times[args.warmup:]), int(tracker.n_live.item()))
        yield {"bench": "klt_video_epipolar", "shape": name, "width": width, "height": height, "max_features": n, "hypotheses": 512,
               "frame_us_median": medians["plain"][0], "frame_with_filter_us_median": medians["filtered"][0],
               "filter_adds_us": round(medians["filtered"][0] - medians["plain"][0], 1), "live": medians["plain"][1], "live_with_filter": medians["filtered"][1]}


def main():
    ap = parser("--repeats", 30, 5)
    ap.add_argument("--frames", type=int, default=30)
    args = ap.parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=True, extra={"device": torch.cuda.get_device_name(0)})


if __name__ == "__main__":
    main()
