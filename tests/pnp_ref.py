"""ctypes binding of tests/pnp_ref.c — the scalar CPU restatement of PnpRansac — and the inputs the CPU and GPU tests
share: scenes of landmarks seen by a camera of the pose family of tests/two_view_pose_ref.py, with their ground truth, and the named cases
of the bit-identity checks.

TEST INFRASTRUCTURE ONLY: compiled on first use (tests/ref_build.py's STRICT flags) into a temporary directory; nothing under
feature_tracker_amd/ may import it, and it imports nothing from there.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests import epipolar_ref as E
from tests import two_view_pose_ref as P
from tests.ref_build import compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pnp_ref.c")

TRACKED, LARGE_RESIDUAL = E.TRACKED, E.LARGE_RESIDUAL
CONTRACT = 0
MUTANTS = {"sign_of_p_not_fixed": 1, "a_transposed": 2, "sequential_sum": 3, "y_residual_unscaled": 4, "zero_landmark_rule_omitted": 5}
# Result.trace
TRACE_WINNER, TRACE_SHEPPERD, TRACE_NEGATED, TRACE_DET_NEGATIVE, TRACE_FINAL_NEGATED, TRACE_STEPS, TRACE_STEP0 = range(7)
MAX_STEPS = 16
TRACE_LENGTH = TRACE_STEP0 + MAX_STEPS
STEP_TAKEN, STEP_FEW_INLIERS, STEP_NOT_POSITIVE_DEFINITE, STEP_NOT_FINITE = range(4)
SAMPLE, MODEL_FLOATS, SUMS, TILE = 6, 12, 27, 256
IMAGE, K, K_OTHER = P.IMAGE, P.K, P.K_OTHER
FAMILY, SHEPPERD_POSES, family_pose = P.FAMILY, P.SHEPPERD_POSES, P.family_pose


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("pnp_ref", [_SRC])
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    l.pnp_solve.argtypes = [vp, vp, vp, i32, vp, f32, i32, C.c_uint32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    l.pnp_solve.restype = i32
    return l


class Result:
    """What one call leaves: status (a rewritten copy), pose [7], n_inliers [1], best [1], valid [1], counts [K], models [K, 12], and, of the
    restatement alone, sums [27] (the first refit step's) and trace [22] (which way each data-dependent choice went)."""


def solve(landmarks, uv, status, K=K, hypotheses=512, threshold=1.0, refine_iterations=4, seed=0, variant=CONTRACT) -> Result:
    landmarks = np.ascontiguousarray(landmarks, np.float32).reshape(-1, 3)
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    r = Result()
    r.status = np.array(status, np.uint8, copy=True)
    n, k = len(landmarks), int(hypotheses)
    assert uv.shape == (n, 2) and r.status.shape == (n,)
    k4 = np.array(K, np.float32)
    r.pose, r.n_inliers, r.best, r.valid = np.zeros(7, np.float32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    r.counts, r.models = np.zeros(k, np.int32), np.zeros((k, MODEL_FLOATS), np.float32)
    r.sums, r.trace = np.zeros(SUMS, np.float32), np.zeros(TRACE_LENGTH, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib().pnp_solve(p(landmarks), p(uv), p(r.status), n, p(k4), float(threshold), k, int(seed) & 0xFFFFFFFF, int(refine_iterations), int(variant),
                         p(r.pose), p(r.n_inliers), p(r.best), p(r.valid), p(r.counts), p(r.models), p(r.sums), p(r.trace))
    assert rc == 0
    return r


OUTPUTS = ("pose", "n_inliers", "best", "valid", "status")
HYPOTHESES = ("counts", "models")


def same_results(a, b, outputs=OUTPUTS) -> list:
    """The names of the outputs in which two results differ by a bit."""
    return [name for name in outputs if not E.same(getattr(a, name), getattr(b, name))]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def scene(n, seed, pose=None, noise=0.0, outlier_share=0.0, K=K):
    """Seeded landmarks of E.scene's cube seen by a camera of ``pose`` = (R, t), X_cur = R X + t (None: P.scene_truth()): (landmarks
    [n, 3] float32, uv [n, 2] float32, is_inlier [n], (R, t)).  A landmark is kept when it is at least E.SCENE_MIN_DEPTH deep and 5 px
    inside the image.  ``noise``: Gaussian sigma in pixels on the inliers' uv.  The first round(n outlier_share) indices of a seeded
    permutation are gross outliers: uv redrawn in the image at least 4 px from the true projection."""
    return _scene(n, seed, E.pose_key(pose), noise, outlier_share, tuple(K))


@functools.lru_cache(maxsize=None)
def _scene(n, seed, pose, noise, outlier_share, K):
    rng = np.random.default_rng(seed)
    R, t = P.scene_truth(pose)
    fx, fy, cx, cy = K
    H, W = IMAGE
    X, uv = np.zeros((0, 3)), np.zeros((0, 2))
    for _ in range(64):  # (a pose or a camera that sees nothing ends here, not in a loop)
        if len(X) >= n:
            break
        cand = np.array(E.SCENE_CENTRE) + rng.uniform(-E.SCENE_HALF_WIDTH, E.SCENE_HALF_WIDTH, (2 * n + 16, 3))
        Y = cand @ R.T + t
        with np.errstate(all="ignore"):
            p = np.c_[fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy]
        seen = (Y[:, 2] >= E.SCENE_MIN_DEPTH) & (p[:, 0] >= 5) & (p[:, 0] <= W - 5) & (p[:, 1] >= 5) & (p[:, 1] <= H - 5)
        X, uv = np.r_[X, cand[seen]], np.r_[uv, p[seen]]
    assert len(X) >= n, "the camera sees too little of the cube"
    X, uv = X[:n], uv[:n].copy()
    is_inlier = np.ones(n, bool)
    is_inlier[rng.permutation(n)[:int(round(n * outlier_share))]] = False
    if noise > 0:
        uv[is_inlier] += rng.normal(0.0, noise, (int(is_inlier.sum()), 2))
    for i in np.flatnonzero(~is_inlier):
        while True:
            cand = rng.uniform([5, 5], [W - 5, H - 5])
            if np.hypot(*(cand - uv[i])) >= 4.0:
                uv[i] = cand
                break
    out = X.astype(np.float32), uv.astype(np.float32), is_inlier
    for a in out:
        a.setflags(write=False)
    return out + ((R, t),)


def family_scene(name, n=300, seed=1, noise=0.0, outlier_share=0.0, K=K):
    return scene(n, seed, family_pose(name), noise, outlier_share, K)


def family_case(name, n=300, noise=0.0, K=K):
    """(landmarks, uv, status) of a family pose, every point a participant: seed 1 at 300 points; another size is the first n points of the
    scene of seed 100 + n."""
    X, uv, _, _ = family_scene(name, 300, 1, noise, K=K) if n == 300 else family_scene(name, max(n, 16), 100 + n, noise, K=K)
    return X[:n].copy(), uv[:n].copy(), np.full(n, TRACKED, np.uint8)


def case(name):
    """name -> (landmarks, uv, status): "n<k>" a scene of that many points, "n<k>_half" with every second row a non-participant of each
    other status in turn; "big<k>": every 97th row out; "full<k>": every row a participant; "zeros": rows with a (0, 0, 0) landmark and
    status TRACKED among real ones; "hostile": NaN, +-inf and 1e30 in landmarks and pixels of TRACKED rows; "identical": one landmark and
    one pixel in every row; "coplanar": every landmark on the plane Z = 6; "behind": every landmark behind the camera that sees it."""
    if name.startswith("big") or name.startswith("full"):
        n = int(name.lstrip("bigful"))
        X, uv, _, _ = scene(n, 400 if name.startswith("big") else 401)
        status = np.full(n, TRACKED, np.uint8)
        if name.startswith("big"):
            status[::97] = E.OUTSIDE
        return X.copy(), uv.copy(), status
    if name.startswith("n"):
        n = int(name[1:].split("_")[0])
        X, uv, _, _ = scene(max(n, 16), 100 + n)
        X, uv = X[:n].copy(), uv[:n].copy()
        status = np.full(n, TRACKED, np.uint8)
        if name.endswith("_half"):
            status[1::2] = np.array([E.NOT_TRACKED, LARGE_RESIDUAL, E.OUTSIDE, E.NUMERIC_ERROR], np.uint8)[np.arange(n // 2) % 4]
        return X, uv, status
    X, uv, _, (R, t) = scene(40, 7)
    X, uv = X.copy(), uv.copy()
    status = np.full(40, TRACKED, np.uint8)
    if name == "zeros":
        X[[0, 5, 6, 21, 39]] = 0.0
    elif name == "hostile":
        X[3, 0], uv[5, 1], X[9, 2], uv[11, 0], X[14], uv[17], X[20, 1], uv[23] = np.nan, np.inf, -np.inf, 1e30, (1e30, -1e30, 1e30), (np.nan, np.nan), 1e30, (-np.inf, 7.0)
    elif name == "identical":
        X[:], uv[:] = X[0], uv[0]
    elif name == "coplanar":
        X[:, 2] = 6.0
        Y = X.astype(np.float64) @ R.T + t
        uv = np.c_[K[0] * Y[:, 0] / Y[:, 2] + K[2], K[1] * Y[:, 1] / Y[:, 2] + K[3]].astype(np.float32)
    elif name == "behind":  # X' with R X' + t = -(R X + t): the same pixels, every depth negative
        X = ((-(X.astype(np.float64) @ R.T + t) - t) @ R).astype(np.float32)
    else:
        raise KeyError(name)
    return X, uv, status


# A camera of 20 px focal length that sees the cube 79 degrees off its axis: every null vector comes out with the sample behind the camera,
# so every model's sign is fixed (on the family's scenes none is: the free column of the elimination is the one of P's last entry).
K_WIDE = (20.0, 20.0, 319.5, 239.5)


def wide_case(n=64):
    X, uv, _, truth = scene(n, 5, pose=(np.eye(3), np.array([-30.0, 0.0, 0.0])), K=K_WIDE)
    return X.copy(), uv.copy(), np.full(n, TRACKED, np.uint8), truth


SIZE_CASES = ("n5", "n6", "n7", "n64_half", "n255", "n256", "n257", "n1025", "big65536", "full65536")
HOSTILE_CASES = ("zeros", "hostile", "identical", "coplanar", "behind")


def three_views(n, seed, pose1, pose2, noise=0.0, outlier_share=0.0, K=K):
    """Landmarks of E.scene's cube seen by three cameras: the reference (identity), ``pose1`` and ``pose2`` (each (R, t), X_cur = R X + t):
    (uv0, uv1, uv2 [n, 2] float32, is_inlier [n], X [n, 3] float64).  Kept when at least E.SCENE_MIN_DEPTH deep and 5 px inside all
    three images.  The outliers' pixels in views 1 and 2 are redrawn in the image."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    H, W = IMAGE
    poses = ((np.eye(3), np.zeros(3)), pose1, pose2)
    X, uvs = np.zeros((0, 3)), [np.zeros((0, 2))] * 3
    while len(X) < n:
        cand = np.array(E.SCENE_CENTRE) + rng.uniform(-E.SCENE_HALF_WIDTH, E.SCENE_HALF_WIDTH, (4 * n + 16, 3))
        seen, views = np.ones(len(cand), bool), []
        for R, t in poses:
            Y = cand @ np.asarray(R).T + np.asarray(t)
            with np.errstate(all="ignore"):
                p = np.c_[fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy]
            seen &= (Y[:, 2] >= E.SCENE_MIN_DEPTH) & (p[:, 0] >= 5) & (p[:, 0] <= W - 5) & (p[:, 1] >= 5) & (p[:, 1] <= H - 5)
            views.append(p)
        X, uvs = np.r_[X, cand[seen]], [np.r_[a, b[seen]] for a, b in zip(uvs, views)]
    X, uvs = X[:n], [a[:n].copy() for a in uvs]
    is_inlier = np.ones(n, bool)
    is_inlier[rng.permutation(n)[:int(round(n * outlier_share))]] = False
    for uv in uvs[1:]:
        if noise > 0:
            uv[is_inlier] += rng.normal(0.0, noise, (int(is_inlier.sum()), 2))
        uv[~is_inlier] = rng.uniform([5, 5], [W - 5, H - 5], (int((~is_inlier).sum()), 2))
    return tuple(a.astype(np.float32) for a in uvs) + (is_inlier, X)
