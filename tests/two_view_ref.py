"""ctypes binding of tests/two_view_ref.c — the scalar CPU restatement of two-view outlier rejection with a choice of model (DESIGN.md
5.21) — and the inputs the CPU and GPU tests share: the planar scenes with a moving patch, and the cases of tests/epipolar_ref.py.

TEST INFRASTRUCTURE ONLY: compiled on first use (gcc -O3 -ffp-contract=off) into a temporary directory; nothing under
feature_tracker_amd/ may import it, and it imports nothing from there.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests import epipolar_ref as E
from tests.ref_build import compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "two_view_ref.c")

TRACKED, LARGE_RESIDUAL = E.TRACKED, E.LARGE_RESIDUAL
FUNDAMENTAL, HOMOGRAPHY, AUTO = 0, 1, 2
MODES = {"fundamental": FUNDAMENTAL, "homography": HOMOGRAPHY, "auto": AUTO}
CONTRACT = 0
MUTANTS = {"transfer_error_with_h_transposed": 1, "dlt_rows_wrong_sign": 2, "auto_rule_counts_swapped": 3, "rewrite_with_the_loser": 4,
           "homography_sampler_allows_duplicates": 5}
F_SAMPLE, H_SAMPLE, ATTEMPTS = 8, 4, 16
IMAGE = E.IMAGE


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("two_view_ref", [_SRC])
    vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32
    l.tvr_choose.argtypes = [i32] * 6
    l.tvr_choose.restype = i32
    l.tvr_ransac.argtypes = [vp, vp, vp, i32, i32, i32, C.c_float, i32, u32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    l.tvr_ransac.restype = i32
    return l


class Result:
    """What one call leaves: status (a rewritten copy), model, best [2], n_inliers [2], F and H [3, 3], counts [2, K], models [2, K, 9],
    samples_f [K, 8] and samples_h [K, 4] (point indices)."""


def choose(has_f, has_h, n_f, n_h, permille, variant=CONTRACT) -> int:
    return int(lib().tvr_choose(int(has_f), int(has_h), int(n_f), int(n_h), int(permille), int(variant)))


def ransac(ref_uv, cur_uv, status, image_size, threshold=1.0, hypotheses=512, seed=0, mode=AUTO, permille=750, variant=CONTRACT) -> Result:
    ref_uv = np.ascontiguousarray(ref_uv, np.float32).reshape(-1, 2)
    cur_uv = np.ascontiguousarray(cur_uv, np.float32).reshape(-1, 2)
    r = Result()
    r.status = np.array(status, np.uint8, copy=True)
    n, K = len(ref_uv), int(hypotheses)
    assert cur_uv.shape == ref_uv.shape and r.status.shape == (n,)
    model = np.zeros(1, np.int32)
    r.best, r.n_inliers = np.zeros(2, np.int32), np.zeros(2, np.int32)
    r.F, r.H = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32)
    r.counts, r.models = np.zeros((2, K), np.int32), np.zeros((2, K, 9), np.float32)
    r.samples_f, r.samples_h = np.zeros((K, F_SAMPLE), np.int32), np.zeros((K, H_SAMPLE), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib().tvr_ransac(p(ref_uv), p(cur_uv), p(r.status), n, int(image_size[0]), int(image_size[1]), float(threshold), K, int(seed) & 0xFFFFFFFF,
                          int(MODES.get(mode, mode)), int(permille), int(variant), p(model), p(r.best), p(r.n_inliers), p(r.F), p(r.H), p(r.counts),
                          p(r.models), p(r.samples_f), p(r.samples_h))
    assert rc == 0
    r.model = int(model[0])
    return r


OUTPUTS = ("status", "best", "n_inliers", "F", "H", "counts", "models")


def same_results(a, b) -> list:
    """The names of the outputs in which two results differ by a bit."""
    bad = [name for name in OUTPUTS if not E.same(getattr(a, name), getattr(b, name))]
    return bad + (["model"] if a.model != b.model else [])


def sample_indices(status, hypotheses, seed, draws=H_SAMPLE):
    """[K, draws] point indices of every hypothesis' draws by the Python restatement of the sampler (tests/epipolar_ref.py's mix32), -1
    from the first draw that ran out of attempts on (all -1 with M < draws)."""
    parts = np.flatnonzero(np.asarray(status) == TRACKED)
    m = len(parts)
    out = np.full((hypotheses, draws), -1, np.int32)
    if m < draws:
        return out
    for h in range(hypotheses):
        drawn = []
        for k in range(draws):
            for a in range(ATTEMPTS):
                j = (E.mix32(seed & 0xFFFFFFFF, h, k, a) * m) >> 32
                if j not in drawn:
                    drawn.append(j)
                    break
            else:
                break
            out[h, k] = parts[j]
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

PATCH_BOX = (380.0, 150.0, 520.0, 290.0)  # (u0, v0, u1, v1) of the patch in the reference image
PATCH_SHIFT = (5.6, -4.2)                 # 7 px on top of the background's motion


def planar_scene(n, seed, camera="moving", noise=0.0, patch_share=0.15, image=IMAGE, pose=None):
    """Scene A: one plane seen by a camera that translates and rolls ("moving") or does not move at all ("static"): (ref_uv, cur_uv,
    on_patch, H64).  The first round(n * patch_share) points lie in PATCH_BOX and move a further PATCH_SHIFT; the others lie outside it.
    ``noise``: Gaussian sigma in pixels on every cur.  ``pose`` = (R, t) with X_cur = R X_ref + t replaces the moving camera's motion; the
    plane then passes through tests/epipolar_ref.py's SCENE_CENTRE, and a point is kept when it is SCENE_MIN_DEPTH deep in both views and
    5 px inside the current image (a patch point: with its shift)."""
    return _planar_scene(n, seed, camera, noise, patch_share, image, E.pose_key(pose))


@functools.lru_cache(maxsize=None)
def _planar_scene(n, seed, camera, noise, patch_share, image, pose):
    rng = np.random.default_rng(seed)
    Hh, W = image
    f = 0.8 * W
    Kc = np.array([[f, 0, 0.5 * (W - 1)], [0, f, 0.5 * (Hh - 1)], [0, 0, 1.0]])
    seen = lambda uv, patch: True  # noqa: E731
    if pose is not None:
        assert camera == "moving"
        R, t = np.array(pose[0]).reshape(3, 3), np.array(pose[1])
        normal = np.array([0.1, -0.2, 1.0]) / np.linalg.norm([0.1, -0.2, 1.0])
        d = float(normal @ np.array(E.SCENE_CENTRE))
        H = Kc @ (R + np.outer(t, normal) / d) @ np.linalg.inv(Kc)

        def seen(uv, patch):
            ray = np.linalg.inv(Kc) @ np.array([uv[0], uv[1], 1.0])
            X = ray * (d / (normal @ ray))
            Y = R @ X + t
            if X[2] < E.SCENE_MIN_DEPTH or Y[2] < E.SCENE_MIN_DEPTH:
                return False
            x2 = (Kc @ Y)[:2] / Y[2] + (np.array(PATCH_SHIFT) if patch else 0.0)
            return 5 <= x2[0] <= W - 5 and 5 <= x2[1] <= Hh - 5
    elif camera == "moving":
        roll = 0.02
        R = np.array([[np.cos(roll), -np.sin(roll), 0], [np.sin(roll), np.cos(roll), 0], [0, 0, 1.0]])
        t, normal, d = np.array([0.3, 0.05, 0.1]), np.array([0.1, -0.2, 1.0]), 5.0
        normal = normal / np.linalg.norm(normal)
        H = Kc @ (R + np.outer(t, normal) / d) @ np.linalg.inv(Kc)
    else:
        assert camera == "static"
        H = np.eye(3)
    n_patch = int(round(n * patch_share))
    u0, v0, u1, v1 = PATCH_BOX
    ref = np.zeros((n, 2))
    k = draws = 0
    while k < n:
        draws += 1
        assert draws <= 1000 * n, "the pose leaves too little of the plane in view"
        if k < n_patch:
            uv = rng.uniform([u0, v0], [u1, v1])
        else:
            uv = rng.uniform([10, 10], [W - 10, Hh - 10])
            if u0 - 2 <= uv[0] <= u1 + 2 and v0 - 2 <= uv[1] <= v1 + 2:
                continue
        if not seen(uv, k < n_patch):
            continue
        ref[k] = uv
        k += 1
    x = (H @ np.c_[ref, np.ones(n)].T).T
    cur = x[:, :2] / x[:, 2:]
    on_patch = np.arange(n) < n_patch
    cur[on_patch] += np.array(PATCH_SHIFT)
    if noise > 0:
        cur += rng.normal(0.0, noise, (n, 2))
    order = rng.permutation(n)  # the patch is not the first indices
    ref, cur, on_patch = ref[order], cur[order], on_patch[order]
    out = ref.astype(np.float32), cur.astype(np.float32), on_patch, H / np.linalg.norm(H)
    for a in out:
        a.setflags(write=False)
    return out


def case(name):
    """name -> (ref_uv, cur_uv, status, image_size): tests/epipolar_ref.py's cases, and "plane<n>": a planar scene of n points, camera
    moving, noise 0.3."""
    if name.startswith("plane"):
        n = int(name[5:])
        ref, cur, _, _ = planar_scene(max(n, 16), 200 + n, "moving", 0.3)
        return ref[:n].copy(), cur[:n].copy(), np.full(n, TRACKED, np.uint8), IMAGE
    return E.case(name)


HOSTILE_CASES = E.HOSTILE_CASES
