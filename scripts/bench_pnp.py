"""Time of PnpRansac.solve at 300 and 2 000 landmarks with 512 and 2 048 hypotheses, with the same contract in stock torch ops (a batched
torch.linalg.svd for the hypotheses, torch.linalg.solve for the refit) timed in the same run as the yardstick.
The torch composition is a different algorithm at ties and rounds differently: a yardstick for time only.  Calls are interleaved in one
process and the medians of device-synchronised wall times are reported, one JSON line per shape (appended to --out, default
profiles/pnp_bench.jsonl).  ``--sample dlt6,p3p`` times both samplers of DESIGN.md 5.30a in the same interleaved rounds and writes one line
per shape and sampler, with a ``sample`` field.  No time is asserted anywhere."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_scenes import K, landmark_scene  # noqa: E402
from scripts.benchlib import interleaved, parser, us_fields, write_rows  # noqa: E402


def torch_pnp(torch, X, uv, status, samples, threshold, refine):
    """The contract in stock torch ops, everything on the device, nothing read back: ``samples`` [K, 6] are drawn once outside (torch
    has no counterpart of the sampler)."""
    fx, fy, cx, cy = K
    xy = torch.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy], 1)
    S, s_xy = X[samples], xy[samples]  # [K, 6, 3], [K, 6, 2]
    mean = S.mean(1, keepdim=True)
    scale = (S - mean).abs().mean((1, 2), keepdim=True)
    Sn = torch.cat([(S - mean) / scale, torch.ones_like(S[:, :, :1])], 2)
    zero = torch.zeros_like(Sn)
    rows = torch.stack([torch.cat([Sn, zero, -s_xy[:, :, :1] * Sn], 2), torch.cat([zero, Sn, -s_xy[:, :, 1:] * Sn], 2)], 2).reshape(len(samples), 12, 12)
    _, _, Vt = torch.linalg.svd(rows[:, :11])
    Pn = Vt[:, -1].reshape(-1, 3, 4)
    A = Pn[:, :, :3] / scale
    b = Pn[:, :, 3] - (A @ mean.transpose(1, 2))[:, :, 0]
    P = torch.cat([A, b[:, :, None]], 2)
    P = P * torch.sign((P[:, 2:3, :3] @ S[:, 0, :, None])[:, :, 0] + P[:, 2:3, 3])[:, :, None]
    Xh = torch.cat([X, torch.ones_like(X[:, :1])], 1)
    c = torch.einsum("kij,nj->kni", P, Xh)
    err2 = (fx * (c[:, :, 0] / c[:, :, 2] - xy[None, :, 0])) ** 2 + (fy * (c[:, :, 1] / c[:, :, 2] - xy[None, :, 1])) ** 2
    part = status == 1
    inl = (c[:, :, 2] > 0) & (err2 <= threshold * threshold) & part[None]
    best = torch.argmax(inl.sum(1))
    U, sv, Vt = torch.linalg.svd(P[best, :, :3])
    R = U @ torch.diag(torch.stack([sv.new_ones(()), sv.new_ones(()), torch.linalg.det(U @ Vt)])) @ Vt
    t = P[best, :, 3] / sv.mean()
    Rrc, p = R.T, -(R.T @ t)
    take = inl[best]
    eye = torch.eye(3, device=X.device)
    for _ in range(refine):
        c = (X - p) @ Rrc
        iz = 1.0 / c[:, 2]
        a_, b_ = c[:, 0] * iz, c[:, 1] * iz
        o = torch.zeros_like(a_)
        J = torch.stack([torch.stack([a_ * b_, -(1 + a_ * a_), b_, -iz, o, a_ * iz], 1), torch.stack([1 + b_ * b_, -a_ * b_, -a_, o, -iz, b_ * iz], 1)], 1)
        res = torch.stack([a_ - xy[:, 0], b_ - xy[:, 1]], 1)
        w = take.to(X.dtype)[:, None, None]
        H = ((J * w).transpose(1, 2) @ J).sum(0)
        g = ((J * w).transpose(1, 2) @ res[:, :, None]).sum(0)[:, 0]
        d = torch.linalg.solve(H, -g)
        skew = torch.stack([torch.stack([o[0], -d[2], d[1]]), torch.stack([d[2], o[0], -d[0]]), torch.stack([-d[1], d[0], o[0]])])
        Rrc, p = Rrc @ (eye + skew), p + Rrc @ d[3:]
        c = (X - p) @ Rrc
        take = (c[:, 2] > 0) & part & ((fx * (c[:, 0] / c[:, 2] - xy[:, 0])) ** 2 + (fy * (c[:, 1] / c[:, 2] - xy[:, 1])) ** 2 <= threshold * threshold)
    status.copy_(torch.where(part & ~take, torch.full_like(status, 2), status))
    return Rrc, p


def rows(args, torch):
    import feature_tracker_amd as F

    for n in (300, 2000):
        X, uv = landmark_scene(n)
        d_X, d_uv = torch.from_numpy(X).cuda(), torch.from_numpy(uv).cuda()
        fresh = torch.ones(n, dtype=torch.uint8, device="cuda")
        for hypotheses in (512, 2048):
            pnps = {name: F.PnpRansac(K, hypotheses=hypotheses, threshold=1.0, refine_iterations=4, seed=1, sample=name) for name in args.sample.split(",")}
            status = fresh.clone()
            samples = torch.from_numpy(np.stack([np.random.default_rng(h).permutation(n)[:6] for h in range(hypotheses)])).cuda()

            def solve(pnp):
                status.copy_(fresh)
                return pnp.solve(d_X, d_uv, status)

            def torch_solve():
                status.copy_(fresh)
                return torch_pnp(torch, d_X, d_uv, status, samples, 1.0, 4)

            calls = {name: (lambda pnp=pnp: solve(pnp)) for name, pnp in pnps.items()}
            calls["torch_solve"] = torch_solve
            times = interleaved(torch, calls, args.repeats, args.warmup)
            for sample, pnp in pnps.items():
                fit = solve(pnp)
                row = {"bench": "pnp", "sample": sample, "points": n, "hypotheses": hypotheses, "refine_iterations": 4, "launches": 13,
                       "n_inliers": int(fit.n_inliers.item()), "valid": int(fit.valid.item())}
                us_fields(row, "solve", times[sample])
                us_fields(row, "torch_solve", times["torch_solve"])
                yield row


def main():
    ap = parser("--repeats", 30, 5, os.path.join(ROOT, "profiles", "pnp_bench.jsonl"))
    ap.add_argument("--sample", default="dlt6", help="the samplers to time in the same rounds, comma-separated: dlt6, p3p")
    args = ap.parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=True, extra={"device": torch.cuda.get_device_name(0)})


if __name__ == "__main__":
    main()
