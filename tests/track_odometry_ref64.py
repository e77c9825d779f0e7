"""An independent float64 composition of ``TrackOdometry.update`` over a sequence, in numpy: the table's rules written
from the contract's text, the triangulation of tests/landmark_table_ref64.py (``lstsq`` midpoint, projection with the division), the pose of
every steady frame from tests/pnp_ref64.py (SVD null vectors, SVD rotation), and, for the bootstrap pair, the TRUE relative pose scaled to the
baseline: there is no float64 two-view filter and pose stage to import, so this composition says what the table and PnP do on a scene given a perfect
first pair.  tests/test_track_odometry_cpu.py checks the sequence's conditions on it before it holds the float32 restatement to them.

TEST INFRASTRUCTURE ONLY.  It shares no code with tests/landmark_table_ref.c; it reads no file of the package.
"""
from __future__ import annotations

import numpy as np

from tests import epipolar_ref as E
from tests import landmark_table_ref64 as L
from tests import pnp_ref64 as P64

IDENTITY = np.array([1.0, 0, 0, 0, 0, 0, 0])


def _rotation(q):
    return L._rotation(q)


def _pose_of(R, t):
    """(R, t) of X_cam = R X + t -> (q_rc with w >= 0, p_rc); rotations here are never near a half turn."""
    M = np.asarray(R, np.float64).T
    w = np.sqrt(max(1e-300, 1.0 + M[0, 0] + M[1, 1] + M[2, 2])) / 2.0
    q = np.array([w, (M[2, 1] - M[1, 2]) / (4 * w), (M[0, 2] - M[2, 0]) / (4 * w), (M[1, 0] - M[0, 1]) / (4 * w)])
    return np.r_[q / np.linalg.norm(q), -M @ np.asarray(t, np.float64)]


class Odometry64:
    def __init__(self, K, threshold=1.0, min_parallax_deg=1.0, min_landmarks=30, baseline=1.0, hypotheses=128, refine_iterations=4, seed=0, rule_c=True):
        self.K, self.threshold, self.min_parallax_deg, self.min_landmarks, self.baseline = tuple(float(k) for k in K), threshold, min_parallax_deg, min_landmarks, baseline
        self.hypotheses, self.refine_iterations, self.seed, self.rule_c = hypotheses, refine_iterations, seed, rule_c
        self.initialised, self.frame, self.anchored, self.scale = False, 0, False, None
        self.owner = None

    def _allocate(self, n):
        self.owner = np.full(n, -1, np.int64)
        self.landmarks, self.anchor_uv, self.anchor_pose = np.zeros((n, 3)), np.zeros((n, 2)), np.zeros((n, 7))
        self.anchor_frame = np.full(n, -1, np.int64)
        self.pose, self.valid, self.lost, self.n_new, self.n_dropped = IDENTITY.copy(), 1, 0, 0, 0
        self.origin = None  # the true pose of the anchor camera

    def holds(self):
        return (self.landmarks != 0).any(1)

    def _slots(self, ids, uv, pose, steady, dropped):
        """Rules a to c for one valid frame."""
        self.pose, self.valid, self.lost, self.n_new, self.n_dropped = pose, 1, 0, 0, 0
        for s in np.flatnonzero(ids >= 0):
            holds, anchored = bool(self.landmarks[s].any()), self.anchor_frame[s] >= 0
            if steady and dropped[s]:
                self.landmarks[s], holds, anchored = 0.0, False, False
                self.n_dropped += 1
            anchor_now = steady and not holds and not anchored
            if not holds and anchored and (self.rule_c or not steady):
                outcome, _, X, _ = L.triangulate(self.anchor_pose[s], self.anchor_uv[s], pose, uv[s], self.K, self.threshold, self.min_parallax_deg)
                if outcome == L.KEPT:
                    self.landmarks[s] = X
                    self.n_new += 1
                elif outcome == L.FAILS and steady:
                    anchor_now = True
            if anchor_now:
                self.anchor_uv[s], self.anchor_pose[s], self.anchor_frame[s] = uv[s], pose, self.frame

    def update(self, ids, points, true_pose):
        """``true_pose``: this frame's (q_rc, p_rc) in the sequence's world, float64; used for the bootstrap pair alone."""
        ids, uv = np.asarray(ids, np.int64), np.asarray(points, np.float64)
        if self.owner is None:
            self._allocate(len(ids))
        changed = ids != self.owner
        self.owner = ids.copy()
        self.landmarks[changed], self.anchor_frame[changed] = 0.0, -1
        none = np.zeros(len(ids), bool)
        if self.initialised:
            status = np.where((ids >= 0) & self.holds(), E.TRACKED, E.NOT_TRACKED)
            fit = P64.solve(self.landmarks, uv, status, self.K, self.hypotheses, self.threshold, self.refine_iterations, self.seed + self.frame)
            if fit.valid == 1:
                dropped = none.copy()
                dropped[fit.participants] = ~fit.kept[fit.participants]
                self._slots(ids, uv, _pose_of(fit.R, fit.t), True, dropped)
            else:
                self.valid, self.lost = -1, self.lost + 1
        elif not self.anchored:
            self.origin = np.asarray(true_pose, np.float64)
            self._slots(ids, uv, IDENTITY.copy(), True, none)
            self.anchored = True
        else:
            R0, R1 = _rotation(self.origin[:4]), _rotation(true_pose[:4])
            p = R0.T @ (true_pose[4:] - self.origin[4:])  # this camera in the anchor camera's frame
            length = float(np.linalg.norm(p))
            if length > 0:
                pose = _pose_of((R0.T @ R1).T, -(R0.T @ R1).T @ (p * self.baseline / length))
                self._slots(ids, uv, pose, False, none)
                n_anchored = int(((ids >= 0) & (self.anchor_frame >= 0)).sum())
                if self.n_new >= self.min_landmarks:
                    self.initialised, self.scale = True, length / self.baseline
                else:
                    self.landmarks[:] = 0.0
                    self.pose = IDENTITY.copy()
                    if n_anchored < self.min_landmarks:
                        self.anchor_frame[:] = -1
                        self.origin = np.asarray(true_pose, np.float64)
                        self._slots(ids, uv, IDENTITY.copy(), True, none)
        self.frame += 1
        return self
