"""Time of TwoViewPose.solve at 300 and 2 000 participants, alone and after TwoViewRansac.filter, with the same contract in stock torch
ops (torch.linalg.eigh, svd, element-wise triangulation) timed in the same run as the yardstick.  The torch
composition is a different algorithm at ties and rounds differently: a yardstick for time only.  Calls are interleaved in one process and the
medians of device-synchronised wall times are reported, one JSON line per shape (appended to --out, default
profiles/two_view_pose_bench.jsonl).  No time is asserted anywhere."""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_scenes import IMAGE, K, two_view_scene  # noqa: E402
from scripts.benchlib import interleaved, parser, us_fields, write_rows  # noqa: E402


def torch_pose(torch, ref_uv, cur_uv, status, threshold, baseline):
    """The contract in stock torch ops: everything on the device, nothing read back (participants by weights, not by a gather)."""
    fx, fy, cx, cy = K
    w = (status == 1).to(torch.float32)
    x1 = torch.stack([(ref_uv[:, 0] - cx) / fx, (ref_uv[:, 1] - cy) / fy, torch.ones_like(w)], 1)
    x2 = torch.stack([(cur_uv[:, 0] - cx) / fx, (cur_uv[:, 1] - cy) / fy, torch.ones_like(w)], 1)
    rows = (x2[:, :, None] * x1[:, None, :]).reshape(-1, 9) * w[:, None]
    _, vec = torch.linalg.eigh(rows.T @ rows)
    U, _, Vt = torch.linalg.svd(vec[:, 0].reshape(3, 3))
    U = U * torch.sign(torch.linalg.det(U))
    Vt = Vt * torch.sign(torch.linalg.det(Vt))
    W = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], device=ref_uv.device)
    Rs = torch.stack([U @ W @ Vt, U @ W @ Vt, U @ W.T @ Vt, U @ W.T @ Vt])
    ts = torch.stack([U[:, 2], -U[:, 2], U[:, 2], -U[:, 2]])
    a = torch.einsum("cij,nj->cni", Rs, x1)
    aa, bb, ab = (a * a).sum(2), (x2 * x2).sum(1)[None], (a * x2[None]).sum(2)
    at, bt = torch.einsum("cni,ci->cn", a, ts), torch.einsum("ni,ci->cn", x2, ts)
    det = aa * bb - ab * ab
    z1, z2 = (ab * bt - bb * at) / det, (aa * bt - ab * at) / det
    front = (z1 > 0) & (z2 > 0) & (w[None] > 0)
    win = torch.argmax(front.sum(1))
    R, t, z = Rs[win], ts[win], z1[win]
    X = z[:, None] * a[win] + t
    err2 = (fx * (X[:, 0] - x2[:, 0] * X[:, 2])) ** 2 + (fy * (X[:, 1] - x2[:, 1] * X[:, 2])) ** 2
    keep = front[win] & (err2 <= threshold * threshold * X[:, 2] ** 2)
    points = torch.where(keep[:, None], baseline * z[:, None] * x1, torch.zeros_like(x1))
    status.copy_(torch.where((w > 0) & ~keep, torch.full_like(status, 2), status))
    return R.T, -(R.T @ t) * baseline, points


def rows(args, torch):
    import feature_tracker_amd as F

    for M in (300, 2000):
        n = int(round(M / 0.7))  # 30 % of the scene are outliers: the filter leaves about M participants
        ref, cur = two_view_scene(n)
        d_ref, d_cur = torch.from_numpy(ref).cuda(), torch.from_numpy(cur).cuda()
        fresh = torch.ones(n, dtype=torch.uint8, device="cuda")
        ransac = F.TwoViewRansac("fundamental", hypotheses=512, threshold=1.0, seed=1)
        filtered = fresh.clone()
        ransac.filter(d_ref, d_cur, filtered, IMAGE)
        pose = F.TwoViewPose(K, threshold=1.0)
        status = fresh.clone()

        def solve_alone():
            status.copy_(filtered)
            return pose.solve(d_ref, d_cur, status)

        def filter_then_solve():
            status.copy_(fresh)
            ransac.filter(d_ref, d_cur, status, IMAGE)
            return pose.solve(d_ref, d_cur, status)

        def filter_alone():
            status.copy_(fresh)
            return ransac.filter(d_ref, d_cur, status, IMAGE)

        def torch_alone():
            status.copy_(filtered)
            return torch_pose(torch, d_ref, d_cur, status, 1.0, 1.0)

        calls = {"solve": solve_alone, "filter": filter_alone, "filter_solve": filter_then_solve, "torch_solve": torch_alone}
        times = interleaved(torch, calls, args.repeats, args.warmup)
        fit = solve_alone()
        row = {"bench": "two_view_pose", "points": n, "participants": int((filtered == 1).sum().item()), "n_points": int(fit.n_points.item()),
               "valid": int(fit.valid.item())}
        for name in calls:
            us_fields(row, name, times[name])
        yield row


def main():
    args = parser("--repeats", 30, 5, os.path.join(ROOT, "profiles", "two_view_pose_bench.jsonl")).parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=True, extra={"device": torch.cuda.get_device_name(0)})


if __name__ == "__main__":
    main()
