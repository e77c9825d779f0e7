"""An independent float64 statement of the landmark table's triangulation, in numpy: the least-squares two-ray midpoint by
``numpy.linalg.lstsq`` (no normal equations), the parallax from the angle between the rays, and a projection test with the division.
tests/test_track_odometry_cpu.py holds tests/landmark_table_ref.c to it.

TEST INFRASTRUCTURE ONLY.  It shares no code with the restatement; it reads no file of the package.
"""
from __future__ import annotations

import numpy as np

WAITS, FAILS, KEPT = 0, 1, 2
REASON_NONE, REASON_NOT_FINITE, REASON_PARALLAX, REASON_DEPTH, REASON_PROJECTION = range(5)


def _rotation(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _pixel_error(pose, X, uv, K):
    c = _rotation(pose[:4]).T @ (X - pose[4:])
    if not c[2] > 0:
        return np.inf, c[2]
    return float(np.hypot(K[0] * c[0] / c[2] + K[2] - uv[0], K[1] * c[1] / c[2] + K[3] - uv[1])), c[2]


def triangulate(pose_a, uv_a, pose_c, uv_c, K, threshold=1.0, min_parallax_deg=1.0):
    """One slot: (outcome, reason, X, margins) with margins = dict(parallax: degrees above the floor, depth: the smaller depth, reprojection:
    threshold minus the larger pixel error); float64 throughout."""
    pose_a, pose_c = np.asarray(pose_a, np.float64), np.asarray(pose_c, np.float64)
    uv_a, uv_c = np.asarray(uv_a, np.float64), np.asarray(uv_c, np.float64)
    X, margins = np.zeros(3), {}
    if not (np.isfinite(pose_a).all() and np.isfinite(pose_c).all() and np.isfinite(uv_a).all() and np.isfinite(uv_c).all()):
        return FAILS, REASON_NOT_FINITE, X, margins
    a = _rotation(pose_a[:4]) @ np.array([(uv_a[0] - K[2]) / K[0], (uv_a[1] - K[3]) / K[1], 1.0])
    b = _rotation(pose_c[:4]) @ np.array([(uv_c[0] - K[2]) / K[0], (uv_c[1] - K[3]) / K[1], 1.0])
    cosine = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
    angle = np.degrees(np.arccos(min(1.0, abs(cosine))))  # the contract compares squares: a ray pair beyond 90 degrees counts by its supplement
    margins["parallax"] = angle - min_parallax_deg
    if angle < min_parallax_deg:
        return WAITS, REASON_PARALLAX, X, margins
    z = np.linalg.lstsq(np.c_[a, -b], pose_c[4:] - pose_a[4:], rcond=None)[0]  # p_a + z1 a ~ p_c + z2 b
    margins["depth"] = float(z.min())
    if not (np.isfinite(z).all() and (z > 0).all()):
        return FAILS, REASON_DEPTH, X, margins
    X = 0.5 * ((pose_a[4:] + z[0] * a) + (pose_c[4:] + z[1] * b))
    ea, _ = _pixel_error(pose_a, X, uv_a, K)
    ec, _ = _pixel_error(pose_c, X, uv_c, K)
    margins["reprojection"] = threshold - max(ea, ec)
    if not (np.isfinite(X).all() and X.any() and max(ea, ec) <= threshold):
        return FAILS, REASON_PROJECTION, X, margins
    return KEPT, REASON_NONE, X, margins
