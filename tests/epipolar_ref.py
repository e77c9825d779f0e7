"""ctypes binding of tests/epipolar_ref.c — the scalar CPU restatement of two-view outlier rejection — and the inputs the
CPU and GPU tests share: synthetic two-view scenes, hostile coordinates, a separate Python restatement of the sampler.

TEST INFRASTRUCTURE ONLY: compiled on first use (gcc -O3 -ffp-contract=off) into a temporary directory; nothing under
feature_tracker_amd/ may import it, and it imports nothing from there.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests.ref_build import compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "epipolar_ref.c")

NOT_TRACKED, TRACKED, LARGE_RESIDUAL, OUTSIDE, NUMERIC_ERROR = range(5)
CONTRACT = 0
MUTANTS = {"highest_h_on_a_tie": 1, "f_applied_transposed": 2, "sampler_allows_duplicates": 3, "threshold_unscaled": 4, "non_participants_sampled": 5}
SAMPLE, ATTEMPTS = 8, 16


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("epipolar_ref", [_SRC])
    vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32
    l.epr_mix32.argtypes = [u32, u32, u32, u32]
    l.epr_mix32.restype = u32
    l.epr_ransac.argtypes = [vp, vp, vp, i32, i32, i32, C.c_float, i32, u32, i32, vp, vp, vp, vp, vp, vp]
    l.epr_ransac.restype = i32
    return l


class Result:
    """What one call leaves: status (a rewritten copy), best, n_inliers, F [3, 3], counts [K], models [K, 9], samples [K, 8] (point indices)."""


def ransac(ref_uv, cur_uv, status, image_size, threshold=1.0, hypotheses=512, seed=0, variant=CONTRACT) -> Result:
    ref_uv = np.ascontiguousarray(ref_uv, np.float32).reshape(-1, 2)
    cur_uv = np.ascontiguousarray(cur_uv, np.float32).reshape(-1, 2)
    r = Result()
    r.status = np.array(status, np.uint8, copy=True)
    n, K = len(ref_uv), int(hypotheses)
    assert cur_uv.shape == ref_uv.shape and r.status.shape == (n,)
    best, n_inliers = np.zeros(1, np.int32), np.zeros(1, np.int32)
    r.F = np.zeros((3, 3), np.float32)
    r.counts, r.models, r.samples = np.zeros(K, np.int32), np.zeros((K, 9), np.float32), np.zeros((K, SAMPLE), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib().epr_ransac(p(ref_uv), p(cur_uv), p(r.status), n, int(image_size[0]), int(image_size[1]), float(threshold), K, int(seed) & 0xFFFFFFFF,
                          int(variant), p(best), p(n_inliers), p(r.F), p(r.counts), p(r.models), p(r.samples))
    assert rc == 0
    r.best, r.n_inliers = int(best[0]), int(n_inliers[0])
    return r


def same(a, b) -> bool:
    """Bit-identical arrays (floats compared as their words)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return bool(np.array_equal(a, b))


# ---- the sampler, restated apart from the C (pure integer logic) ------------------------------------------------------

_M32 = 0xFFFFFFFF


def _fmix32(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & _M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & _M32
    x ^= x >> 16
    return x


def mix32(seed, h, k, a):
    return _fmix32(_fmix32((seed + 0x9E3779B9 * (h + 1)) & _M32) ^ ((0x85EBCA6B * (k * ATTEMPTS + a + 1)) & _M32))


def sample_indices(status, hypotheses, seed):
    """[K, 8] point indices of every hypothesis' draws, -1 from the first draw that ran out of attempts on (all -1 with M < 8)."""
    parts = np.flatnonzero(np.asarray(status) == TRACKED)
    m = len(parts)
    out = np.full((hypotheses, SAMPLE), -1, np.int32)
    if m < SAMPLE:
        return out
    for h in range(hypotheses):
        drawn = []
        for k in range(SAMPLE):
            for a in range(ATTEMPTS):
                j = (mix32(seed & _M32, h, k, a) * m) >> 32
                if j not in drawn:
                    drawn.append(j)
                    break
            else:
                break
            out[h, k] = parts[j]
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

IMAGE = (480, 640)  # (H, W)


SCENE_CENTRE = (0.0, 0.0, 6.0)  # scenes with a given pose: points in a cube of half-width SCENE_HALF_WIDTH about this point of the reference frame
SCENE_HALF_WIDTH = 1.5
SCENE_MIN_DEPTH = 0.5           # ... kept when at least this deep in both views and 5 px inside both images


def pose_key(pose):
    """(R, t) -> a hashable key of its float64 values (None stays None): what the cached scene functions take."""
    if pose is None:
        return None
    R, t = pose
    return tuple(float(v) for v in np.asarray(R, np.float64).reshape(9)), tuple(float(v) for v in np.asarray(t, np.float64).reshape(3))


def scene(n, seed, outlier_share=0.3, noise=0.0, image=IMAGE, min_outlier_distance=4.0, pose=None):
    """Seeded 3-D points seen by two pinhole poses with real translation: (ref_uv, cur_uv, is_inlier, F64).  The first
    round(n * outlier_share) indices of a seeded permutation are gross outliers: cur is redrawn until it lies at least
    ``min_outlier_distance`` pixels from the true epipolar line of ref.  ``noise``: Gaussian sigma in pixels on the inliers' cur.
    ``pose`` = (R, t) with X_cur = R X_ref + t: None is the one small motion these scenes began with (points by pixel and depth 2-10); a
    given pose sees points of the cube about SCENE_CENTRE."""
    return _scene(n, seed, outlier_share, noise, image, min_outlier_distance, pose_key(pose))


@functools.lru_cache(maxsize=None)
def _scene(n, seed, outlier_share, noise, image, min_outlier_distance, pose):
    rng = np.random.default_rng(seed)
    H, W = image
    f = 0.8 * W
    Kc = np.array([[f, 0, 0.5 * (W - 1)], [0, f, 0.5 * (H - 1)], [0, 0, 1.0]])
    ref, cur = np.zeros((n, 2)), np.zeros((n, 2))
    k = 0
    if pose is None:
        ang = np.array([0.03, -0.05, 0.02])
        Rx = np.array([[1, 0, 0], [0, np.cos(ang[0]), -np.sin(ang[0])], [0, np.sin(ang[0]), np.cos(ang[0])]])
        Ry = np.array([[np.cos(ang[1]), 0, np.sin(ang[1])], [0, 1, 0], [-np.sin(ang[1]), 0, np.cos(ang[1])]])
        Rz = np.array([[np.cos(ang[2]), -np.sin(ang[2]), 0], [np.sin(ang[2]), np.cos(ang[2]), 0], [0, 0, 1]])
        R, t = Rz @ Ry @ Rx, np.array([0.5, 0.1, 0.15])
        while k < n:
            uv = rng.uniform([10, 10], [W - 10, H - 10])
            depth = rng.uniform(2.0, 10.0)
            X = np.linalg.inv(Kc) @ np.array([uv[0], uv[1], 1.0]) * depth
            x2 = Kc @ (R @ X + t)
            x2 = x2[:2] / x2[2]
            if 5 <= x2[0] <= W - 5 and 5 <= x2[1] <= H - 5:
                ref[k], cur[k] = uv, x2
                k += 1
    else:
        R, t = np.array(pose[0]).reshape(3, 3), np.array(pose[1])
        while k < n:
            X = np.array(SCENE_CENTRE) + rng.uniform(-SCENE_HALF_WIDTH, SCENE_HALF_WIDTH, 3)
            Y = R @ X + t
            if X[2] < SCENE_MIN_DEPTH or Y[2] < SCENE_MIN_DEPTH:
                continue
            x1, x2 = Kc @ X, Kc @ Y
            x1, x2 = x1[:2] / x1[2], x2[:2] / x2[2]
            if all(5 <= x[0] <= W - 5 and 5 <= x[1] <= H - 5 for x in (x1, x2)):
                ref[k], cur[k] = x1, x2
                k += 1
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = np.linalg.inv(Kc).T @ tx @ R @ np.linalg.inv(Kc)
    F /= np.linalg.norm(F)
    is_inlier = np.ones(n, bool)
    is_inlier[rng.permutation(n)[:int(round(n * outlier_share))]] = False
    if noise > 0:
        cur[is_inlier] += rng.normal(0.0, noise, (int(is_inlier.sum()), 2))
    for i in np.flatnonzero(~is_inlier):
        line = F @ np.array([ref[i, 0], ref[i, 1], 1.0])
        while True:
            cand = rng.uniform([5, 5], [W - 5, H - 5])
            if abs(line @ np.array([cand[0], cand[1], 1.0])) / np.hypot(line[0], line[1]) >= min_outlier_distance:
                cur[i] = cand
                break
    for a in (ref, cur, is_inlier, F):
        a.setflags(write=False)
    return ref.astype(np.float32), cur.astype(np.float32), is_inlier, F


def case(name):
    """name -> (ref_uv, cur_uv, status, image_size): the inputs of the bit-identity checks, CPU and GPU."""
    if name.startswith("n"):  # "n257": a scene of that many points; "n64_half": every other point is no participant
        n = int(name[1:].split("_")[0])
        ref, cur, _, _ = scene(max(n, 16), 100 + n)
        ref, cur = ref[:n].copy(), cur[:n].copy()
        status = np.full(n, TRACKED, np.uint8)
        if name.endswith("_half"):
            status[1::2] = np.array([NOT_TRACKED, LARGE_RESIDUAL, OUTSIDE, NUMERIC_ERROR], np.uint8)[np.arange(n // 2) % 4]
        return ref, cur, status, IMAGE
    ref, cur, _, _ = scene(40, 7)
    ref, cur = ref.copy(), cur.copy()
    status = np.full(40, TRACKED, np.uint8)
    if name == "identical":  # every participant the same point: every matrix has rank 1, every hypothesis is invalid
        ref[:], cur[:] = ref[0], cur[0]
    elif name == "hostile":  # NaN, inf and 1e30 among the participants
        ref[3, 0], cur[5, 1], ref[9, 1], cur[11, 0], ref[14], cur[17] = np.nan, np.inf, -np.inf, 1e30, (1e30, -1e30), (np.nan, np.nan)
    elif name == "interleaved":
        status[::3] = OUTSIDE
        status[1::7] = NOT_TRACKED
        ref[::3] = np.nan  # what a non-participant holds must not matter
    elif name == "collinear":  # all points on one image line in both views: rank-deficient, zero pivots
        ref[:, 1], cur[:, 1] = 100.0, 120.0
    else:
        raise KeyError(name)
    return ref, cur, status, IMAGE


HOSTILE_CASES = ("identical", "hostile", "interleaved", "collinear")
