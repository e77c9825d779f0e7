"""ctypes binding of tests/pnp_p3p_ref.c — the scalar CPU restatement of PnpRansac's "p3p" sampler.  The inputs are
tests/pnp_ref.py's; this module adds the planar scene and the samples the solver is driven with alone.

TEST INFRASTRUCTURE ONLY: compiled on first use (tests/ref_build.py's STRICT flags) into a temporary directory; nothing under
feature_tracker_amd/ may import it, and it imports nothing from there.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests import epipolar_ref as E
from tests import pnp_ref as R
from tests.ref_build import compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pnp_p3p_ref.c")

CONTRACT = 0
MUTANTS = {"fourth_point_ignored": 1, "front_of_the_sample_not_tested": 2, "tie_takes_the_last": 3, "y_error_unscaled": 4, "one_newton_step_fewer": 5}
SAMPLE, REFIT_MIN, CUBIC_STEPS, NEWTON_STEPS = 4, 6, 64, 1


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("pnp_p3p_ref", [_SRC])
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    l.pnp_p3p_solve.argtypes = [vp, vp, vp, i32, vp, f32, i32, C.c_uint32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    l.pnp_p3p_solve.restype = i32
    l.p3p_solve.argtypes = [vp, vp, i32, vp]
    l.p3p_solve.restype = i32
    l.p3p_hypothesis.argtypes = [vp, f32, i32, vp, vp]
    l.p3p_hypothesis.restype = i32
    l.p3p_choose.argtypes = [vp, i32, i32]
    l.p3p_choose.restype = i32
    return l


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def solve(landmarks, uv, status, K=R.K, hypotheses=512, threshold=1.0, refine_iterations=4, seed=0, variant=CONTRACT) -> R.Result:
    """pnp_ref.solve's arguments and Result under the "p3p" sampler, and ``solutions`` [K]: how many poses the solver returned for each
    hypothesis (-1: no draw, or a degenerate sample)."""
    landmarks = np.ascontiguousarray(landmarks, np.float32).reshape(-1, 3)
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    r = R.Result()
    r.status = np.array(status, np.uint8, copy=True)
    n, k = len(landmarks), int(hypotheses)
    assert uv.shape == (n, 2) and r.status.shape == (n,)
    k4 = np.array(K, np.float32)
    r.pose, r.n_inliers, r.best, r.valid = np.zeros(7, np.float32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    r.counts, r.models = np.zeros(k, np.int32), np.zeros((k, R.MODEL_FLOATS), np.float32)
    r.sums, r.trace, r.solutions = np.zeros(R.SUMS, np.float32), np.zeros(R.TRACE_LENGTH, np.int32), np.zeros(k, np.int32)
    rc = lib().pnp_p3p_solve(_p(landmarks), _p(uv), _p(r.status), n, _p(k4), float(threshold), k, int(seed) & 0xFFFFFFFF, int(refine_iterations),
                             int(variant), _p(r.pose), _p(r.n_inliers), _p(r.best), _p(r.valid), _p(r.counts), _p(r.models), _p(r.sums), _p(r.trace),
                             _p(r.solutions))
    assert rc == 0
    return r


def solver(xy, X, variant=CONTRACT):
    """The solver alone: calibrated pixels [3, 2] and landmarks [3, 3] -> (count, solutions [count, 3, 4]); count -1: degenerate."""
    xy, X = np.ascontiguousarray(xy, np.float32).reshape(3, 2), np.ascontiguousarray(X, np.float32).reshape(3, 3)
    sols = np.zeros((4, 3, 4), np.float32)
    count = lib().p3p_solve(_p(xy), _p(X), int(variant), _p(sols))
    return count, sols[:max(count, 0)]


def hypothesis(xy, X, ry=1.0, variant=CONTRACT):
    """One hypothesis of four participants: (valid, [R | t] [3, 4], the solver's count)."""
    rows = np.ascontiguousarray(np.c_[np.asarray(xy, np.float32).reshape(4, 2), np.asarray(X, np.float32).reshape(4, 3)], np.float32)
    P, count = np.zeros((3, 4), np.float32), np.zeros(1, np.int32)
    ok = lib().p3p_hypothesis(_p(rows), float(ry), int(variant), _p(P), _p(count))
    return bool(ok), P, int(count[0])


def choose(errors, variant=CONTRACT) -> int:
    """The choice among candidates by their errors at the fourth point alone."""
    errors = np.ascontiguousarray(errors, np.float32)
    return int(lib().p3p_choose(_p(errors), len(errors), int(variant)))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

def calibrated(uv, K=R.K):
    """float32 (x, y) as the scan computes them."""
    k = np.array(K, np.float32)
    uv = np.asarray(uv, np.float32)
    return np.stack([(uv[:, 0] - k[2]) / k[0], (uv[:, 1] - k[3]) / k[1]], 1)


@functools.lru_cache(maxsize=None)
def tilted_plane(n=300, seed=11, outlier_share=0.3, tilt_degrees=30.0):
    """Landmarks of one plane through the scene's centre, tilted about the x axis, seen by P.scene_truth()'s camera: (landmarks, uv,
    is_inlier, (R, t)), outliers as pnp_ref.scene's."""
    rng = np.random.default_rng(seed)
    Rt, t = R.P.scene_truth(None)
    fx, fy, cx, cy = R.K
    H, W = R.IMAGE
    a = np.deg2rad(tilt_degrees)
    e1, e2 = np.array([1.0, 0.0, 0.0]), np.array([0.0, np.cos(a), np.sin(a)])
    X, uv = np.zeros((0, 3)), np.zeros((0, 2))
    for _ in range(64):
        if len(X) >= n:
            break
        st = rng.uniform(-E.SCENE_HALF_WIDTH, E.SCENE_HALF_WIDTH, (2 * n + 16, 2))
        cand = np.array(E.SCENE_CENTRE) + st[:, :1] * e1 + st[:, 1:] * e2
        Y = cand @ Rt.T + t
        p = np.c_[fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy]
        seen = (Y[:, 2] >= E.SCENE_MIN_DEPTH) & (p[:, 0] >= 5) & (p[:, 0] <= W - 5) & (p[:, 1] >= 5) & (p[:, 1] <= H - 5)
        X, uv = np.r_[X, cand[seen]], np.r_[uv, p[seen]]
    assert len(X) >= n
    X, uv = X[:n], uv[:n].copy()
    is_inlier = np.ones(n, bool)
    is_inlier[rng.permutation(n)[:int(round(n * outlier_share))]] = False
    for i in np.flatnonzero(~is_inlier):
        while True:
            cand = rng.uniform([5, 5], [W - 5, H - 5])
            if np.hypot(*(cand - uv[i])) >= 4.0:
                uv[i] = cand
                break
    return X.astype(np.float32), uv.astype(np.float32), is_inlier, (Rt, t)


def coplanar_truth():
    """The pose of pnp_ref.case("coplanar")'s camera."""
    return R.scene(40, 7)[3]


def case(name):
    """pnp_ref.case's names, and "collinear" (every landmark on one line, at steps that float32 holds exactly, seen where it projects) and "coincident" (every odd row a copy
    of the row before it: a sample that draws both holds two coincident landmarks)."""
    if name not in ("collinear", "coincident"):
        return R.case(name)
    X, uv, _, (Rt, t) = R.scene(40, 7)
    X, uv = X.copy(), uv.copy()
    if name == "collinear":
        X = (np.array(E.SCENE_CENTRE) + ((np.arange(40) - 20) / 16.0)[:, None] * np.array([1.0, 0.5, 0.25])).astype(np.float32)
        Y = X.astype(np.float64) @ Rt.T + t
        uv = np.c_[R.K[0] * Y[:, 0] / Y[:, 2] + R.K[2], R.K[1] * Y[:, 1] / Y[:, 2] + R.K[3]].astype(np.float32)
    else:
        X[1::2], uv[1::2] = X[0::2], uv[0::2]
    return X, uv, np.full(40, R.TRACKED, np.uint8)


SIZE_CASES = ("n3", "n4", "n5", "n6", "n7", "n64_half", "n255", "n256", "n257", "n1025", "full65536")
NAMED_CASES = ("zeros", "hostile", "identical", "behind", "collinear", "coincident", "coplanar")
