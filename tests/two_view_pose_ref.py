"""ctypes binding of tests/two_view_pose_ref.c — the scalar CPU restatement of TwoViewPose — and the inputs the CPU and GPU
tests share: the two-view scenes of tests/epipolar_ref.py with their ground truth, and the named cases of the bit-identity checks.

TEST INFRASTRUCTURE ONLY: compiled on first use (tests/ref_build.py's STRICT flags) into a temporary directory; nothing under
feature_tracker_amd/ may import it, and it imports nothing from there.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests import epipolar_ref as E
from tests.ref_build import compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "two_view_pose_ref.c")

TRACKED, LARGE_RESIDUAL = E.TRACKED, E.LARGE_RESIDUAL
CONTRACT = 0
MUTANTS = {"twisted_pair_chosen": 1, "t_with_the_wrong_sign": 2, "e_transposed": 3, "sequential_sum": 4, "reprojection_unscaled_by_fx": 5}
# mutants of the quaternion's branches that the scenes of one small rotation never reach: only the pose family (below) catches them
FAMILY_MUTANTS = {"shepperd_x_branch_sign": 6, "shepperd_y_branch_sign": 7, "shepperd_z_branch_sign": 8, "negation_to_w_positive_omitted": 9}
# Result.trace: the choices (-1 where the call ended before one), then the pairs of either Jacobi by the path they took
TRACE_K, TRACE_K2, TRACE_I1, TRACE_I2, TRACE_WINNER, TRACE_SHEPPERD, TRACE_NEGATED = range(7)
TRACE_JACOBI9, TRACE_JACOBI3, TRACE_LENGTH = slice(7, 12), slice(12, 17), 17
JACOBI_PATHS = ("zero", "negligible", "apq_over_h", "theta_positive", "theta_negative")
SWEEPS = 7  # FTK_POSE_JACOBI_SWEEPS (include/ftk.h): S + 1 with the S of DESIGN.md 5.29
IMAGE = E.IMAGE
K = (0.8 * IMAGE[1], 0.8 * IMAGE[1], 0.5 * (IMAGE[1] - 1), 0.5 * (IMAGE[0] - 1))  # the camera of E.scene: (fx, fy, cx, cy)
K_OTHER = (470.0, 455.0, 300.5, 251.25)  # a second camera for the current view


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("two_view_pose_ref", [_SRC])
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    l.tvp_solve.argtypes = [vp, vp, vp, i32, vp, f32, f32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    l.tvp_solve.restype = i32
    return l


class Result:
    """What one call leaves: status (a rewritten copy), pose [7], points [n, 3], E [3, 3], n_front [4], valid [1], n_points [1], and A [45]
    (the moment sums, row-major upper triangle), trace [17] (the restatement alone: which way each data-dependent choice went)."""


def solve(ref_uv, cur_uv, status, K=K, K_cur=None, threshold=1.0, baseline=1.0, sweeps=SWEEPS, variant=CONTRACT) -> Result:
    ref_uv = np.ascontiguousarray(ref_uv, np.float32).reshape(-1, 2)
    cur_uv = np.ascontiguousarray(cur_uv, np.float32).reshape(-1, 2)
    r = Result()
    r.status = np.array(status, np.uint8, copy=True)
    n = len(ref_uv)
    assert cur_uv.shape == ref_uv.shape and r.status.shape == (n,)
    k8 = np.array(tuple(K) + tuple(K if K_cur is None else K_cur), np.float32)
    r.pose, r.points, r.E = np.zeros(7, np.float32), np.zeros((n, 3), np.float32), np.zeros((3, 3), np.float32)
    r.n_front, r.valid, r.n_points, r.A = np.zeros(4, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(45, np.float32)
    r.trace = np.zeros(TRACE_LENGTH, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib().tvp_solve(p(ref_uv), p(cur_uv), p(r.status), n, p(k8), float(threshold), float(baseline), int(sweeps), int(variant), p(r.pose), p(r.points),
                         p(r.E), p(r.n_front), p(r.valid), p(r.n_points), p(r.A), p(r.trace))
    assert rc == 0
    return r


OUTPUTS = ("pose", "E", "n_front", "valid", "n_points", "points", "status")


def same_results(a, b, outputs=OUTPUTS) -> list:
    """The names of the outputs in which two results differ by a bit."""
    return [name for name in outputs if not E.same(getattr(a, name), getattr(b, name))]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def rotation(axis, degrees):
    """Rodrigues' rotation matrix, float64."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    S = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    w = np.deg2rad(degrees)
    return np.eye(3) + np.sin(w) * S + (1.0 - np.cos(w)) * (S @ S)


# The pose family: every rotation with every offset, the camera turning about the middle of the points it sees:
# X_cur = R (X_ref - c) + c + off, so t = c + off - R c.  The 170-degree turns have one diagonal entry of R near +1 and two near -1 (each of
# Shepperd's three other branches), the turns by 130 to 150 degrees have a negative trace with a negative w before the negation.
ROTATIONS = {"small": ((1, -2, 1), 3.4), "x170": ((1, .05, .02), 170), "y170": ((.03, 1, .04), 170), "z170": ((.02, .03, 1), 170),
             "y130": ((0, 1, .1), 130), "z-150": ((.1, 0, 1), -150), "x-140": ((1, .1, 0), -140), "z90": ((0, 0, 1), 90)}
OFFSETS = {"side": (.6, .1, .2), "back": (-.5, .3, -.4), "forward": (.02, .01, .8)}  # forward: the epipole lies inside the image
FAMILY = tuple(f"{r}/{o}" for r in ROTATIONS for o in OFFSETS)
SHEPPERD_BRANCH = {"small": 0, "z90": 0, "x170": 1, "x-140": 1, "y170": 2, "y130": 2, "z170": 3, "z-150": 3}  # asserted from the trace
SHEPPERD_POSES = ("small/side", "x170/side", "y170/back", "z170/side")  # one pose per branch of the quaternion, 0 ... 3
# The same at nine points.  Ten of the 24 nine-point cuts fall below the rank floor and are refused (small, z170 and z90 at every offset,
# z-150/side: tests/test_two_view_pose_cpu.py asserts which and why the floor cannot move): branch 0 has no valid nine-point cut in the family
# (small/side stands for it, refused; the case n9 of the older scenes is its valid one), branch 3 has z-150/back.
SHEPPERD_POSES_N9 = ("small/side", "x170/side", "y170/back", "z-150/back")
# What the two-view filters are held to the restatements on, on the device: a pose per branch, a forward pose with inliers about the epipole, and
# small/forward, where the winning sample holds an outlier (tests/test_epipolar_cpu.py runs the whole family and says what the bound there is).
FILTER_POSES = SHEPPERD_POSES + ("x170/forward", "small/forward")
# Below this float64 ratio of the second-smallest to the largest eigenvalue of the inliers' A, a scene has a second fundamental matrix that
# fits every inlier within a pixel, and a filter that counts inliers may keep an outlier through which a mix of the two passes.  The family has
# no scene between 6.6e-6 (z170/back) and 1.18e-5 (z-150/forward); the value is the power of ten between them.
FILTER_WELL_CONDITIONED = 1.0e-5


def family_pose(name):
    """"x170/side" -> (R, t), float64."""
    rot, off = name.split("/")
    R, c = rotation(*ROTATIONS[rot]), np.array(E.SCENE_CENTRE)
    return R, c + np.array(OFFSETS[off]) - R @ c


def family_scene(name, n=300, seed=1, noise=0.0, outlier_share=0.0):
    """E.scene of a family pose: (ref_uv, cur_uv, is_inlier, F64)."""
    return E.scene(n, seed, outlier_share=outlier_share, noise=noise, pose=family_pose(name))


def family_case(name, n=300, noise=0.0):
    """(ref_uv, cur_uv, status) of a family pose, every point a participant: seed 1 at 300 points; another size is the first n points of
    the scene of seed 100 + n, as in case()."""
    ref, cur, _, _ = family_scene(name, 300, 1, noise) if n == 300 else family_scene(name, max(n, 16), 100 + n, noise)
    return ref[:n].copy(), cur[:n].copy(), np.full(n, TRACKED, np.uint8)


def scene_truth(pose=None):
    """(R, t) of E.scene: X_cur = R X_ref + t, float64."""
    if pose is not None:
        return np.array(pose[0], np.float64).reshape(3, 3), np.array(pose[1], np.float64).reshape(3)
    ang = np.array([0.03, -0.05, 0.02])
    Rx = np.array([[1, 0, 0], [0, np.cos(ang[0]), -np.sin(ang[0])], [0, np.sin(ang[0]), np.cos(ang[0])]])
    Ry = np.array([[np.cos(ang[1]), 0, np.sin(ang[1])], [0, 1, 0], [-np.sin(ang[1]), 0, np.cos(ang[1])]])
    Rz = np.array([[np.cos(ang[2]), -np.sin(ang[2]), 0], [np.sin(ang[2]), np.cos(ang[2]), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx, np.array([0.5, 0.1, 0.15])


def big_scene(n, seed, pose=None):
    """n correspondences of the camera pair of E.scene without its rejection loop (vectorised: the 65 536-point case): (ref_uv, cur_uv).
    With a pose: the points of E.scene's cube, drawn in blocks of 2 n and the first n visible ones kept."""
    return _big_scene(n, seed, E.pose_key(pose))


@functools.lru_cache(maxsize=None)
def _big_scene(n, seed, pose):
    rng = np.random.default_rng(seed)
    R, t = scene_truth(pose)
    fx, fy, cx, cy = K
    if pose is None:
        uv = rng.uniform([60, 60], [IMAGE[1] - 60, IMAGE[0] - 60], (n, 2))
        depth = rng.uniform(2.0, 10.0, n)
        X = np.c_[(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(n)] * depth[:, None]
        Y = X @ R.T + t
        cur = np.c_[fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy]
    else:
        uv, cur = np.zeros((0, 2)), np.zeros((0, 2))
        while len(uv) < n:
            X = np.array(E.SCENE_CENTRE) + rng.uniform(-E.SCENE_HALF_WIDTH, E.SCENE_HALF_WIDTH, (2 * n, 3))
            Y = X @ R.T + t
            with np.errstate(all="ignore"):
                a = np.c_[fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy]
                b = np.c_[fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy]
            inside = lambda p: (p[:, 0] >= 5) & (p[:, 0] <= IMAGE[1] - 5) & (p[:, 1] >= 5) & (p[:, 1] <= IMAGE[0] - 5)  # noqa: E731
            seen = (X[:, 2] >= E.SCENE_MIN_DEPTH) & (Y[:, 2] >= E.SCENE_MIN_DEPTH) & inside(a) & inside(b)
            uv, cur = np.r_[uv, a[seen]], np.r_[cur, b[seen]]
        uv, cur = uv[:n], cur[:n]
    out = uv.astype(np.float32), cur.astype(np.float32)
    for a in out:
        a.setflags(write=False)
    return out


def case(name):
    """name -> (ref_uv, cur_uv, status): "n<k>" / "n<k>_half" / the hostile cases as in tests/epipolar_ref.py (scenes without outliers:
    the participants are what a filter left); "big<k>": big_scene with every 97th point no participant (at k = 65 536: M = 64 860, 254
    tiles, the last two workgroups of the grid idle); "full<k>": big_scene with every point a participant (at k = 65 536: every scan
    thread's 64-bit mask full, 256 full tiles); "hostile_finite": NaN and inf among the participants, no 1e30."""
    if name.startswith("big"):
        n = int(name[3:])
        ref, cur = big_scene(n, 400)
        status = np.full(n, TRACKED, np.uint8)
        status[::97] = E.OUTSIDE
        return ref.copy(), cur.copy(), status
    if name.startswith("full"):
        n = int(name[4:])
        ref, cur = big_scene(n, 401)
        return ref.copy(), cur.copy(), np.full(n, TRACKED, np.uint8)
    if name.startswith("n"):
        n = int(name[1:].split("_")[0])
        ref, cur, _, _ = E.scene(max(n, 16), 100 + n, outlier_share=0.0)
        ref, cur = ref[:n].copy(), cur[:n].copy()
        status = np.full(n, TRACKED, np.uint8)
        if name.endswith("_half"):
            status[1::2] = np.array([E.NOT_TRACKED, LARGE_RESIDUAL, E.OUTSIDE, E.NUMERIC_ERROR], np.uint8)[np.arange(n // 2) % 4]
        return ref, cur, status
    ref, cur, _, _ = E.scene(40, 7, outlier_share=0.0)
    ref, cur = ref.copy(), cur.copy()
    status = np.full(40, TRACKED, np.uint8)
    if name.startswith("squeezed"):  # towards one image line in both views by s / 100: either side of the rank test's floor (15, 20)
        s = np.float32(int(name[8:]) / 100.0)
        ref[:, 1], cur[:, 1] = 100 + s * (ref[:, 1] - 100), 120 + s * (cur[:, 1] - 120)
    elif name == "identical":
        ref[:], cur[:] = ref[0], cur[0]
    elif name == "hostile":  # 1e30 among the participants: its products overflow float32, the sums are not finite
        ref[3, 0], cur[5, 1], ref[9, 1], cur[11, 0], ref[14], cur[17] = np.nan, np.inf, -np.inf, 1e30, (1e30, -1e30), (np.nan, np.nan)
    elif name == "hostile_finite":
        ref[3, 0], cur[5, 1], ref[9, 1], cur[17] = np.nan, np.inf, -np.inf, (np.nan, np.nan)
    elif name == "interleaved":
        status[::3] = E.OUTSIDE
        status[1::7] = E.NOT_TRACKED
        ref[::3] = np.nan
    elif name == "collinear":
        ref[:, 1], cur[:, 1] = 100.0, 120.0
    else:
        raise KeyError(name)
    return ref, cur, status


HOSTILE_CASES = ("identical", "hostile", "hostile_finite", "interleaved", "collinear", "squeezed15", "squeezed20")
