"""Time of a steady-state TrackOdometry.update at 300 and 2 000 slots, and of a KltVideoTracker frame with and without ``odometry``, with the
same frame written with what exists without the class as the yardstick, timed in the same run: PnpRansac, the
ownership bookkeeping on the host (ids read back, compared, the landmark array zeroed and uploaded again) and the triangulation in stock
torch ops.  The torch composition rounds differently and anchors by boolean masks: a yardstick for time only.  Calls are interleaved in one
process and the medians of device-synchronised wall times are reported, one JSON line per shape (appended to --out, default
profiles/track_odometry_bench.jsonl).  No time is asserted anywhere; the kernels' own times are not measured here."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_scenes import IMAGE, K  # noqa: E402
from scripts.benchlib import parser, us_median, wall_time, write_rows  # noqa: E402


def sequence(n, frames, seed=1, churn=0.05, outlier_share=0.2, noise=0.3, step=0.1):
    """``frames`` track tables of n slots: (ids int64 [n], points float32 [n, 2]) per frame, from a camera that moves ``step`` per frame
    sideways past points 4.5 to 7.5 deep; each frame ``churn`` of the slots get a fresh id and point; a share of gross outliers."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    ids, next_id = np.arange(n, dtype=np.int64), n
    X = np.array([0.0, 0.0, 6.0]) + rng.uniform(-1.5, 1.5, (n, 3))
    gross = rng.uniform(size=n) < outlier_share
    out = []
    for f in range(frames):
        if f > 0:
            refill = rng.permutation(n)[:int(round(n * churn))]
            ids[refill] = next_id + np.arange(len(refill))
            next_id += len(refill)
            X[refill] = np.array([0.0, 0.0, 6.0]) + rng.uniform(-1.5, 1.5, (len(refill), 3))
            gross[refill] = rng.uniform(size=len(refill)) < outlier_share
        c = X - np.array([1.0, -0.2, 0.25]) * (step * f)
        uv = np.c_[fx * c[:, 0] / c[:, 2] + cx, fy * c[:, 1] / c[:, 2] + cy] + rng.normal(0.0, noise, (n, 2))
        uv[gross] = rng.uniform([5, 5], [IMAGE[1] - 5, IMAGE[0] - 5], (int(gross.sum()), 2))
        out.append((ids.copy(), uv.astype(np.float32)))
    return out


def rotation(torch, q):
    w, x, y, z = q[0], q[1], q[2], q[3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]).reshape(3, 3)


class HandOdometry:
    """The steady-state frame without the class: ownership on the host, PnpRansac, triangulation in stock torch ops."""

    def __init__(self, F, torch, n, threshold=1.0, min_parallax_deg=1.0):
        self.torch, self.pnp, self.threshold = torch, F.PnpRansac(K, threshold=threshold), threshold
        self.c2 = float(np.cos(np.radians(min_parallax_deg)) ** 2)
        self.owner = np.full(n, -1, np.int64)
        self.landmarks = torch.zeros(n, 3, device="cuda")
        self.anchor_uv, self.anchor_pose = torch.zeros(n, 2, device="cuda"), torch.zeros(n, 7, device="cuda")
        self.anchor_frame = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.frame = 0

    def rays(self, uv, poses):
        torch = self.torch
        xy1 = torch.stack([(uv[:, 0] - K[2]) / K[0], (uv[:, 1] - K[3]) / K[1], torch.ones_like(uv[:, 0])], 1)
        q = poses[:, :4]
        w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
        return torch.einsum("nij,nj->ni", R, xy1), R

    def inlier(self, X, R, p, uv):
        c = self.torch.einsum("nji,nj->ni", R, X - p)
        e = (K[0] * c[:, 0] / c[:, 2] + K[2] - uv[:, 0]) ** 2 + (K[1] * c[:, 1] / c[:, 2] + K[3] - uv[:, 1]) ** 2
        return (c[:, 2] > 0) & (e <= self.threshold ** 2)

    def update(self, ids, points):
        torch = self.torch
        host_ids = ids.cpu().numpy()  # the round trip: read ids, compare, zero, upload again
        changed = host_ids != self.owner
        self.owner = host_ids
        lm = self.landmarks.cpu().numpy()
        lm[changed] = 0
        self.landmarks = torch.from_numpy(lm).cuda()
        self.anchor_frame[torch.from_numpy(changed).cuda()] = -1
        live = ids >= 0
        status = (live & (self.landmarks != 0).any(1)).to(torch.uint8)
        fit = self.pnp.solve(self.landmarks, points, status, seed=self.frame)
        dropped = status == 2
        self.landmarks[dropped] = 0
        self.anchor_frame[dropped] = -1
        empty = live & ~(self.landmarks != 0).any(1)
        fresh = empty & (self.anchor_frame < 0)
        pose = fit.pose.expand(len(ids), 7)
        a, Ra = self.rays(self.anchor_uv, self.anchor_pose)
        b, Rc = self.rays(points, pose)
        t = self.anchor_pose[:, 4:] - pose[:, 4:]
        aa, bb, ab, at, bt = (a * a).sum(1), (b * b).sum(1), (a * b).sum(1), (a * t).sum(1), (b * t).sum(1)
        det = aa * bb - ab * ab
        z1, z2 = (ab * bt - bb * at) / det, (aa * bt - ab * at) / det
        X = 0.5 * ((self.anchor_pose[:, 4:] + z1[:, None] * a) + (pose[:, 4:] + z2[:, None] * b))
        tried = empty & ~fresh & ~(ab * ab > self.c2 * (aa * bb))
        kept = tried & (z1 > 0) & (z2 > 0) & self.inlier(X, Ra, self.anchor_pose[:, 4:], self.anchor_uv) & self.inlier(X, Rc, pose[:, 4:], points)
        self.landmarks = torch.where(kept[:, None], X, self.landmarks)
        anchor = fresh | (tried & ~kept)
        self.anchor_uv = torch.where(anchor[:, None], points, self.anchor_uv)
        self.anchor_pose = torch.where(anchor[:, None], pose, self.anchor_pose)
        self.anchor_frame = torch.where(anchor, torch.full_like(self.anchor_frame, self.frame), self.anchor_frame)
        self.frame += 1


def rows(args, torch):
    import feature_tracker_amd as F
    from feature_tracker_amd import device as D
    from feature_tracker_amd import synth

    for n in (300, 2000):
        seq = [(torch.from_numpy(i).cuda(), torch.from_numpy(p).cuda()) for i, p in sequence(n, args.warmup + args.repeats)]
        odo, hand = F.TrackOdometry(K, seed=0), HandOdometry(F, torch, n)
        times = {"update": [], "hand": []}
        for f, (ids, points) in enumerate(seq):
            t_odo = wall_time(torch, lambda: odo.update(ids, points, IMAGE))
            if odo.initialised and f > 0 and hand.frame == 0:  # the yardstick starts from the class's map
                hand.owner = odo.owner.cpu().numpy().copy()
                hand.landmarks, hand.anchor_uv, hand.anchor_pose = odo.landmarks.clone(), odo.anchor_uv.clone(), odo.anchor_pose.clone()
                hand.anchor_frame, hand.frame = odo.anchor_frame.clone(), odo.frame
                continue
            if hand.frame > 0:
                t_hand = wall_time(torch, lambda: hand.update(ids, points))
                if f >= args.warmup:
                    times["update"].append(t_odo)
                    times["hand"].append(t_hand)
        yield {"what": "steady_update", "slots": n, "frames": len(times["update"]), "initialised": bool(odo.initialised), "valid": int(odo.valid[0]),
               "n_landmarks": int(odo.n_landmarks[0]), "launches": 15,
               "update_us_median": us_median(times["update"]), "hand_us_median": us_median(times["hand"])}
    # a KltVideoTracker frame with and without odometry (the tracker's own synthetic frames: one plane, so the odometry stays in its bootstrap)
    frames = [np.ascontiguousarray(synth.make_image_pair(640, 480, (0.7 * k, -0.4 * k))[1]) for k in range(args.warmup + args.repeats)]
    times = {}
    for name in ("tracker", "tracker_with_odometry"):
        ctx = D.context_on_stream(torch.cuda.Stream())
        flow = F.OpticalFlowBasicKlt()
        flow.options().kMethod = "fast"
        flow.options().kMaxTrackPointsNumber = 500
        odo = F.TrackOdometry(K, ctx=ctx) if name.endswith("odometry") else None
        tracker = F.KltVideoTracker(flow, 300, ctx=ctx, odometry=odo)
        images = [torch.from_numpy(f).cuda() for f in frames]
        times[name] = [wall_time(torch, lambda: tracker.track(image)) for image in images][args.warmup:]
    yield {"what": "klt_video_frame", "slots": 300, "image": [480, 640], "frames": args.repeats, "odometry_state": "bootstrap (one plane: the homography is chosen)",
           "tracker_us_median": us_median(times["tracker"]), "tracker_with_odometry_us_median": us_median(times["tracker_with_odometry"])}


def main():
    args = parser("--repeats", 30, 8, os.path.join(ROOT, "profiles", "track_odometry_bench.jsonl")).parse_args()
    import torch

    write_rows(rows(args, torch), args.out, append=True)


if __name__ == "__main__":
    main()
