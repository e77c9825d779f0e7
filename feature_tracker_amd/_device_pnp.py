"""``device.pnp_ransac_device``: the torch device entry of the camera pose from landmarks and their pixels (ftk_pnp_ransac_device,
DESIGN.md 5.30).

It is re-exported by device.py and held to that module's rule: no ``datapointer()`` of a tensor that did not pass ``device._check``.  It lives
in a file of its own for _device_epipolar.py's reason; its walk and its refusals are tests/test_pnp_args_cpu.py.
"""
from __future__ import annotations

import ctypes as C

from . import _native as N
from ._device_two_view_pose import check_camera, check_scalars
from ._torch_call import pointer, stream_or_current


def check_counts(hypotheses, refine_iterations, seed):
    """(hypotheses, refine_iterations, seed) as the ABI takes them, or the ValueError: before anything touches a device."""
    try:
        k, r, s = int(hypotheses), int(refine_iterations), int(seed)
    except (TypeError, ValueError):
        raise ValueError(f"hypotheses, refine_iterations and seed must be integers (got {hypotheses!r}, {refine_iterations!r}, {seed!r})") from None
    if not 1 <= k <= N.FTK_EPIPOLAR_MAX_HYPOTHESES:
        raise ValueError(f"hypotheses must be in 1 .. FTK_EPIPOLAR_MAX_HYPOTHESES = {N.FTK_EPIPOLAR_MAX_HYPOTHESES} (got {hypotheses})")
    if not 0 <= r <= N.FTK_PNP_MAX_REFINE_ITERATIONS:
        raise ValueError(f"refine_iterations must be in 0 .. FTK_PNP_MAX_REFINE_ITERATIONS = {N.FTK_PNP_MAX_REFINE_ITERATIONS} (got {refine_iterations})")
    if not 0 <= s <= 0xFFFFFFFF:
        raise ValueError(f"seed must be a uint32 (got {seed})")
    return k, r, s


SAMPLES = {"dlt6": N.FTK_PNP_SAMPLE_DLT6, "p3p": N.FTK_PNP_SAMPLE_P3P}


def check_sample(sample, name="sample") -> str:
    """The sampler's name, or the ValueError: before anything touches a device."""
    if not isinstance(sample, str) or sample not in SAMPLES:
        raise ValueError(f"{name} must be one of {sorted(SAMPLES)} (got {sample!r})")
    return sample


def pnp_args(ctx, landmarks, uv, status, K, threshold: float, hypotheses: int, refine_iterations: int, seed: int, workspace, pose, n_inliers, best,
             valid, counts=None, models=None, stream=None, sample=None):
    """Checks one ftk_pnp_ransac_device call (``sample`` None) or one ftk_pnp_ransac_sampled_device call and returns its marshalled arguments."""
    from . import device as D

    code = None if sample is None else SAMPLES[check_sample(sample)]
    cam = check_camera("K", K)
    t, _ = check_scalars(threshold, 1.0)
    k, r, s = check_counts(hypotheses, refine_iterations, seed)
    dev = D._call_device(ctx, landmarks)
    D._check("landmarks", landmarks, D._F32, (None, 3), dev)
    n = int(landmarks.shape[0])
    if not 1 <= n <= N.FTK_TRACK_TABLE_MAX_SLOTS:
        raise ValueError(f"landmarks must have 1 .. FTK_TRACK_TABLE_MAX_SLOTS = {N.FTK_TRACK_TABLE_MAX_SLOTS} points (got {n})")
    D._check("uv", uv, D._F32, (n, 2), dev)
    D._check("status", status, D._U8, (n,), dev)
    D._check("workspace", workspace, D._KEYS, (None,), dev, min_numel=-(-N.pnp_ransac_workspace_bytes(n, k, r) // 8))
    D._check("pose", pose, D._F32, (7,), dev)
    D._check("n_inliers", n_inliers, D._I32, (1,), dev)
    D._check("best", best, D._I32, (1,), dev)
    D._check("valid", valid, D._I32, (1,), dev)
    if counts is not None:
        D._check("counts", counts, D._I32, (k,), dev)
    if models is not None:
        D._check("models", models, D._F32, (k, N.FTK_PNP_MODEL_FLOATS), dev)
    st = stream_or_current(landmarks, stream)
    return ((ctx.handle, C.c_void_p(st.cuda_stream), pointer(landmarks), pointer(uv), pointer(status), n) + tuple(C.c_float(e) for e in cam)
            + (C.c_float(t), k, r, C.c_uint32(s)) + (() if code is None else (code,)) + (pointer(workspace), pointer(pose), pointer(n_inliers), pointer(best), pointer(valid), pointer(counts),
               pointer(models)))


def pnp_ransac_device(ctx, landmarks, uv, status, K, threshold: float, hypotheses: int, refine_iterations: int, seed: int, workspace, pose, n_inliers,
                      best, valid, counts=None, models=None, stream=None) -> None:
    """ftk_pnp_ransac_device: the pose of the camera that sees ``landmarks[i]`` (contiguous float32 CUDA [n, 3]) at ``uv[i]`` (float32 [n, 2],
    (u, v) pixels) for the points whose ``status`` (uint8 [n]) is TRACKED, whose five numbers are finite and whose landmark is not
    (0, 0, 0), by the contract of DESIGN.md 5.30: RANSAC over the six-point DLT, then ``refine_iterations`` Gauss-Newton steps on the
    reprojection error of the inliers.  ``K``: (fx, fy, cx, cy).  ``pose`` float32 [7] receives q_rc (w, x, y, z) and p_rc in DirectMethod's
    convention, ``n_inliers`` / ``best`` / ``valid`` int32 [1] the inliers of the final pose, the winning hypothesis and 1 or -1,
    ``counts`` int32 [hypotheses] and ``models`` float32 [hypotheses, 12] every hypothesis when given; ``status`` is rewritten in place (a
    participant that is no inlier of the final pose becomes LARGE_RESIDUAL; nothing changes when the result is invalid).
    ``workspace``: int64 or uint64 CUDA tensor of at least ``_native.pnp_ransac_workspace_bytes(n, hypotheses, refine_iterations) / 8``
    elements, no initialisation needed.  5 + 2 ``refine_iterations`` launches on ``stream`` (default: torch's current stream), no
    synchronisation, no allocation: capturable.  Every argument is checked before the device is touched."""
    args = pnp_args(ctx, landmarks, uv, status, K, threshold, hypotheses, refine_iterations, seed, workspace, pose, n_inliers, best, valid, counts, models,
                    stream)
    N.check(N.lib().ftk_pnp_ransac_device(*args), ctx.handle)


def pnp_ransac_sampled_device(ctx, landmarks, uv, status, K, threshold: float, hypotheses: int, refine_iterations: int, seed: int, sample: str,
                              workspace, pose, n_inliers, best, valid, counts=None, models=None, stream=None) -> None:
    """ftk_pnp_ransac_sampled_device: ``pnp_ransac_device`` with the minimal solver behind the hypotheses chosen by ``sample``: "dlt6" (that
    call exactly) or "p3p" (four participants per hypothesis, three to a P3P solver and the fourth choosing among its
    solutions; ``models`` then holds [R | t]; a call needs 4 participants, and landmarks of one plane give a pose).  Same workspace, same
    launches, same checks; another ``sample`` is a ValueError before the device is touched."""
    args = pnp_args(ctx, landmarks, uv, status, K, threshold, hypotheses, refine_iterations, seed, workspace, pose, n_inliers, best, valid, counts, models,
                    stream, sample=check_sample(sample))
    N.check(N.lib().ftk_pnp_ransac_sampled_device(*args), ctx.handle)
