"""ctypes binding of tests/landmark_table_ref.c — the scalar CPU restatement of the landmark table's two kernels — its
composition with tests/pnp_ref.py, tests/two_view_ref.py and tests/two_view_pose_ref.py into a restatement of ``TrackOdometry.update``,
host decisions included, and the inputs the CPU and GPU tests share: tables in which every branch of the two kernels occurs, and a
sequence of track tables seen by a camera that translates and turns through tests/pnp_ref.py's kind of scene.

TEST INFRASTRUCTURE ONLY: compiled on first use (tests/ref_build.py's STRICT flags) into a temporary directory; nothing under
feature_tracker_amd/ may import it, and it imports nothing from there.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os

import numpy as np

from tests import epipolar_ref as E
from tests import pnp_ref as R
from tests import two_view_pose_ref as P
from tests import two_view_ref as T
from tests.ref_build import compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "landmark_table_ref.c")

NOT_TRACKED, TRACKED, LARGE_RESIDUAL = E.NOT_TRACKED, E.TRACKED, E.LARGE_RESIDUAL
VALID, N_NEW, N_ANCHORED, N_LANDMARKS, N_DROPPED, LOST = range(6)
COUNTERS = 8
STEADY, BOOTSTRAP = 0, 1
CONTRACT = 0
MUTANTS = {"owner_change_keeps_the_landmark": 1, "parallax_test_omitted": 2, "t_with_the_other_sign": 3, "no_reanchor_after_a_failure": 4,
           "landmark_from_one_ray": 5}
RULE_C_OFF = 6  # no mutant: the contrast of the sequence test
O_NONE, O_WAITS, O_FAILS, O_KEPT = -1, 0, 1, 2
IMAGE, K = R.IMAGE, R.K
IDENTITY = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)
STATE = ("owner", "landmarks", "anchor_uv", "anchor_pose", "anchor_frame", "counters", "pose")


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("landmark_table_ref", [_SRC])
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    l.lt_begin.argtypes = [vp, i32] + [vp] * 6 + [i32]
    l.lt_begin.restype = i32
    l.lt_end.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, i32, vp, f32, f32] + [vp] * 6 + [i32, vp]
    l.lt_end.restype = i32
    return l


def cos2(min_parallax_deg) -> float:
    """cos^2 of the parallax floor as the entry receives it: float64 on the host, rounded to float32 once."""
    return float(np.float32(math.cos(math.radians(float(min_parallax_deg))) ** 2))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Table:
    """The table's state for n slots, as ``TrackOdometry`` makes it: no owner, no landmark, no anchor."""

    def __init__(self, n):
        self.owner = np.full(n, -1, np.int64)
        self.landmarks, self.anchor_uv, self.anchor_pose = np.zeros((n, 3), np.float32), np.zeros((n, 2), np.float32), np.zeros((n, 7), np.float32)
        self.anchor_frame = np.full(n, -1, np.int32)
        self.pnp_status, self.anchor_status = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self.counters, self.pose = np.zeros(COUNTERS, np.int32), IDENTITY.copy()

    def copy(self):
        other = Table(0)
        for name, value in vars(self).items():
            setattr(other, name, value.copy())
        return other


def begin(t: Table, ids, variant=CONTRACT) -> None:
    ids = np.ascontiguousarray(ids, np.int64)
    assert lib().lt_begin(_p(ids), len(ids), _p(t.owner), _p(t.landmarks), _p(t.anchor_frame), _p(t.pnp_status), _p(t.anchor_status), _p(t.counters),
                          int(variant)) == 0


def end(t: Table, ids, points, status_in, pose_in, valid_in, model_in, frame, mode, K=K, threshold=1.0, c2=None, variant=CONTRACT):
    """Returns the outcome of rule c per slot (O_NONE: not attempted)."""
    ids, points = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(points, np.float32)
    status_in = None if status_in is None else np.ascontiguousarray(status_in, np.uint8)
    pose_in, valid_in = np.ascontiguousarray(pose_in, np.float32), np.ascontiguousarray(valid_in, np.int32).reshape(1)
    model_in = None if model_in is None else np.ascontiguousarray(model_in, np.int32).reshape(1)
    k4, outcome = np.array(K, np.float32), np.zeros(len(ids), np.int8)
    assert lib().lt_end(_p(ids), _p(points), len(ids), _p(status_in), _p(pose_in), _p(valid_in), _p(model_in), int(frame), int(mode), _p(k4), float(threshold),
                        cos2(1.0) if c2 is None else float(c2), _p(t.landmarks), _p(t.anchor_uv), _p(t.anchor_pose), _p(t.anchor_frame), _p(t.counters),
                        _p(t.pose), int(variant), _p(outcome)) == 0
    return outcome


def same_tables(a: Table, b, names=STATE + ("pnp_status", "anchor_status")) -> list:
    """The names of the state tensors in which two tables (or a table and anything with its attributes) differ by a bit."""
    return [name for name in names if not E.same(np.asarray(getattr(a, name)), np.asarray(getattr(b, name)))]


class Odometry:
    """``TrackOdometry`` restated: the same calls in the same order, the same host decisions, the restatements in place of the entries."""

    def __init__(self, K=K, threshold=1.0, min_parallax_deg=1.0, min_landmarks=30, baseline=1.0, hypotheses=512, refine_iterations=4, seed=0, variant=CONTRACT):
        self.K, self.threshold, self.c2, self.min_landmarks, self.baseline = tuple(K), threshold, cos2(min_parallax_deg), min_landmarks, baseline
        self.hypotheses, self.refine_iterations, self.seed, self.variant = hypotheses, refine_iterations, seed, variant
        self.initialised, self.frame, self._anchored, self.table = False, 0, False, None
        self.outcome = None  # rule c's outcome per slot of the last end call

    def _end(self, ids, points, mode, pose_in, valid_in, model_in=None):
        t = self.table
        self.outcome = end(t, ids, points, t.pnp_status if mode == STEADY else None, pose_in, valid_in, model_in, self.frame, mode, self.K, self.threshold,
                           self.c2, self.variant)

    def _anchor_all(self, ids, points):
        begin(self.table, ids, self.variant)
        self._end(ids, points, STEADY, IDENTITY, [1])
        self._anchored = True

    def update(self, ids, points, image_size=IMAGE):
        ids, points = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(points, np.float32)
        if self.table is None:
            self.table = Table(len(ids))
        t, seed = self.table, (self.seed + self.frame) & 0xFFFFFFFF
        if self.initialised:
            begin(t, ids, self.variant)
            fit = R.solve(t.landmarks, points, t.pnp_status, self.K, self.hypotheses, self.threshold, self.refine_iterations, seed)
            t.pnp_status[:] = fit.status
            self._end(ids, points, STEADY, fit.pose, fit.valid)
        elif not self._anchored:
            self._anchor_all(ids, points)
        else:
            begin(t, ids, self.variant)
            fit = T.ransac(t.anchor_uv, points, t.anchor_status, image_size, self.threshold, self.hypotheses, seed, T.AUTO)
            two = P.solve(t.anchor_uv, points, fit.status, self.K, threshold=self.threshold, baseline=self.baseline)
            t.anchor_status[:] = two.status
            self._end(ids, points, BOOTSTRAP, two.pose, two.valid, [fit.model])
            valid, n_new, n_anchored = (int(v) for v in t.counters[:3])
            if valid == 1 and n_new >= self.min_landmarks:
                self.initialised = True
            else:
                t.landmarks[:] = 0
                t.counters[N_LANDMARKS] = t.counters[N_NEW] = 0
                t.pose[:] = IDENTITY
                if n_anchored < self.min_landmarks:
                    t.anchor_frame[:] = -1
                    self._anchor_all(ids, points)
        self.frame += 1
        return self


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def pose_of(Rcw, tcw):
    """(R, t) of X_cam = R X_world + t, float64 -> (q_rc (w >= 0), p_rc) float64 [7]: R_rc = R^T, p_rc = -R^T t."""
    M = np.asarray(Rcw, np.float64).T
    w = math.sqrt(max(0.0, 1.0 + M[0, 0] + M[1, 1] + M[2, 2])) / 2.0
    if w > 1e-6:
        q = np.array([w, (M[2, 1] - M[1, 2]) / (4 * w), (M[0, 2] - M[2, 0]) / (4 * w), (M[1, 0] - M[0, 1]) / (4 * w)])
    else:  # a half turn: the axis from the largest diagonal entry
        i = int(np.argmax(np.diag(M)))
        v = (M[:, i] + np.eye(3)[i]) / 2.0
        q = np.r_[0.0, v / math.sqrt(v[i])]
    q = q / np.linalg.norm(q)
    return np.r_[q, -M @ np.asarray(tcw, np.float64)]


def rotation_of(q):
    """R_rc of a quaternion (w, x, y, z), float64."""
    w, x, y, z = (float(v) for v in q[:4])
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def project(pose, X, K=K):
    """Pixels of world points X [m, 3] seen from ``pose`` (q_rc, p_rc), float64, and their depths."""
    c = (np.asarray(X, np.float64) - pose[4:]) @ rotation_of(pose)
    with np.errstate(all="ignore"):
        return np.c_[K[0] * c[:, 0] / c[:, 2] + K[2], K[1] * c[:, 1] / c[:, 2] + K[3]], c[:, 2]


def pair_table(name, n=300, seed=1, noise=0.0, K=K):
    """A table whose every slot is anchored at the first pose of the family pair ``name`` (the identity) and seen now from the second:
    (table, ids, points, pose_cur float32 [7], X float64 [n, 3])."""
    ref, cur, _, _ = P.family_scene(name, n, seed, noise)
    Rt = P.family_pose(name)
    X64 = _family_points(name, n, seed)
    t = Table(n)
    ids = np.arange(n, dtype=np.int64)
    t.owner[:], t.anchor_uv[:], t.anchor_pose[:], t.anchor_frame[:] = ids, ref, IDENTITY, 0
    return t, ids, cur.copy(), pose_of(*Rt).astype(np.float32), X64


def _family_points(name, n, seed):
    """The 3-D points of P.family_scene(name, n, seed) in the reference camera, float64: E.scene does not return them, so its draws are
    replayed from the seed (the same generator, the same rejections in the same order), and the replay is checked against its pixels."""
    Rm, tv = P.family_pose(name)
    rng = np.random.default_rng(seed)
    H, W = IMAGE
    out = []
    while len(out) < n:
        X = np.array(E.SCENE_CENTRE) + rng.uniform(-E.SCENE_HALF_WIDTH, E.SCENE_HALF_WIDTH, 3)
        Y = Rm @ X + tv
        if X[2] < E.SCENE_MIN_DEPTH or Y[2] < E.SCENE_MIN_DEPTH:
            continue
        views = [(K[0] * Z[0] / Z[2] + K[2], K[1] * Z[1] / Z[2] + K[3]) for Z in (X, Y)]
        if all(5 <= u <= W - 5 and 5 <= v <= H - 5 for u, v in views):
            out.append(X)
    out = np.array(out)
    ref = P.family_scene(name, n, seed, 0.0)[0]
    assert np.abs(project(IDENTITY.astype(np.float64), out)[0] - ref).max() < 1e-3, "the replay of E.scene's draws left its points"
    return out


BRANCH_SLOTS = ("empty", "changed_owner", "holder", "fresh", "no_anchor", "outlier", "waits", "behind_anchor", "behind_current", "off_anchor", "off_current",
                "not_finite", "triangulates")


def branch_table(n, seed=0):
    """A table of n slots in which every branch of the two kernels occurs, in turn by slot (BRANCH_SLOTS[s % 13]), and the frame's inputs:
    (table, ids, points, status_in, pose_in float32 [7]).  The table is as a begin call of an earlier frame left it, except the slots named
    "changed_owner" (their id is not their owner's: this frame's begin clears them); status_in is what PnpRansac would leave (LARGE_RESIDUAL
    on "outlier").  The camera stands at the identity for the anchors and has moved sideways and turned for the current frame."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    Rm, tv = P.rotation((0.1, 1.0, 0.05), 4.0), np.array([-0.4, 0.05, 0.1])
    cur = pose_of(Rm, tv)
    X = np.array(E.SCENE_CENTRE) + rng.uniform(-E.SCENE_HALF_WIDTH, E.SCENE_HALF_WIDTH, (n, 3))
    uv_a, _ = project(IDENTITY.astype(np.float64), X)
    uv_c, _ = project(cur, X)
    t = Table(n)
    ids = np.arange(n, dtype=np.int64) + 100
    t.owner[:] = ids
    points = uv_c.astype(np.float32)
    status = np.full(n, NOT_TRACKED, np.uint8)
    kind = np.arange(n) % len(BRANCH_SLOTS)
    name = lambda k: kind == BRANCH_SLOTS.index(k)  # noqa: E731
    t.anchor_uv[:], t.anchor_pose[:], t.anchor_frame[:] = uv_a.astype(np.float32), IDENTITY, 3
    ids[name("empty")] = -1
    t.owner[name("empty")] = -1
    t.anchor_frame[name("empty")] = -1
    t.owner[name("changed_owner")] = 7
    t.landmarks[name("changed_owner")] = X[name("changed_owner")]
    for k in ("holder", "outlier"):
        t.landmarks[name(k)] = X[name(k)]
        status[name(k)] = TRACKED if k == "holder" else LARGE_RESIDUAL
    t.anchor_frame[name("no_anchor")] = -1
    t.anchor_frame[name("fresh")] = -1
    t.anchor_uv[name("waits")] = project(IDENTITY.astype(np.float64), X[name("waits")] * 400.0)[0]   # the same ray direction far away: no parallax
    points[name("waits")] = project(cur, X[name("waits")] * 400.0)[0]
    for k, dv in (("behind_anchor", 0.0), ("behind_current", 25.0)):  # rays that diverge: their crossing lies behind the cameras
        m = int(name(k).sum())
        t.anchor_uv[name(k)] = np.c_[np.full(m, K[2] - 120.0), 200.0 + np.arange(m) % 80].astype(np.float32)
        points[name(k)] = np.c_[np.full(m, K[2] + 120.0), 200.0 + dv + np.arange(m) % 80].astype(np.float32)
    t.anchor_uv[name("off_anchor")] += np.array([0.0, 9.0], np.float32)     # across the epipolar line: the midpoint misses both by pixels
    points[name("off_current")] += np.array([0.0, -9.0], np.float32)
    bad = np.flatnonzero(name("not_finite"))
    for j, s in enumerate(bad):
        (points if j % 2 == 0 else t.anchor_uv)[s, j % 2] = (np.nan, np.inf, -np.inf)[j % 3]
    return t, ids, points, status, cur.astype(np.float32)


SEQUENCE_FRAMES, SEQUENCE_SLOTS = 26, 300


@functools.lru_cache(maxsize=None)
def sequence(noise=0.0, seed=11, frames=SEQUENCE_FRAMES, n=SEQUENCE_SLOTS, churn=0.05, outlier_share=0.2, K=K, step=0.06, depth=(3.0, 18.0)):
    """A sequence of track tables: ``frames`` x (ids int64 [n], points float32 [n, 2]), the true pose of every frame (float64 [7], world = the
    first camera), and per frame the set of ids that are gross outliers from birth.  The camera moves ``step`` per frame sideways (a little
    up and forward) and turns 0.35 degrees per frame about an axis near y, past points of a frustum 3 to 18 deep (``depth``; None: E.scene's cube), so that parallax reaches
    the near points first.  Each frame about ``churn`` of the slots
    retire: one in five of them stays empty for that frame, the others come back at once with a fresh id and a fresh point.  A gross
    outlier's pixel is redrawn in the image every frame."""
    rng = np.random.default_rng(seed)
    H, W = IMAGE
    ids = np.arange(n, dtype=np.int64)
    next_id = n
    def draw(m):
        if depth is None:
            return np.array(E.SCENE_CENTRE) + rng.uniform(-E.SCENE_HALF_WIDTH, E.SCENE_HALF_WIDTH, (m, 3))
        z = rng.uniform(depth[0], depth[1], m)  # a frustum: the cube's lateral extent at its centre's depth, scaled with the depth
        xy = rng.uniform(-E.SCENE_HALF_WIDTH, E.SCENE_HALF_WIDTH, (m, 2)) * (z / E.SCENE_CENTRE[2])[:, None]
        return np.c_[xy, z]

    X = draw(n)
    gross = rng.uniform(size=n) < outlier_share
    out_ids, out_points, poses, out_gross = [], [], [], []
    for f in range(frames):
        Rm = P.rotation((0.05, 1.0, 0.02), 0.35 * f)
        centre = np.array([1.0, -0.2, 0.25]) * (step * f)
        pose = pose_of(Rm, -Rm @ centre)
        if f > 0:
            retire = rng.permutation(n)[:int(round(n * churn))]
            empty = retire[::5]
            refill = np.setdiff1d(np.r_[retire, np.flatnonzero(ids < 0)], empty)
            ids[empty] = -1
            ids[refill] = next_id + np.arange(len(refill))
            next_id += len(refill)
            X[refill] = draw(len(refill))
            gross[refill] = rng.uniform(size=len(refill)) < outlier_share
        uv, _ = project(pose, X, K)
        if noise > 0:
            uv = uv + rng.normal(0.0, noise, uv.shape)
        uv[gross] = rng.uniform([5, 5], [W - 5, H - 5], (int(gross.sum()), 2))
        uv[ids < 0] = 0.0
        out_ids.append(ids.copy())
        out_points.append(uv.astype(np.float32))
        poses.append(pose)
        out_gross.append(frozenset(int(i) for i in ids[gross & (ids >= 0)]))
    for a in out_ids + out_points + poses:
        a.setflags(write=False)
    return tuple(out_ids), tuple(out_points), tuple(poses), tuple(out_gross)
