"""``device.two_view_pose_device``: the torch device entry of the relative pose and the landmarks of two-view inliers
(ftk_two_view_pose_device).

It is re-exported by device.py and held to that module's rule: no ``datapointer()`` of a tensor that did not pass ``device._check``.  It lives
in a file of its own for _device_epipolar.py's reason; its walk and its refusals are tests/test_two_view_pose_args_cpu.py.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _native as N
from ._torch_call import pointer, stream_or_current


def _f32(x) -> float:
    """``x`` as the ABI's float32 receives it (rounded; an overflow is inf, an underflow 0)."""
    return C.c_float(float(x)).value


def check_camera(name, K):
    """(fx, fy, cx, cy) as the ABI receives them (float32), fx and fy finite and > 0, cx and cy finite, or the ValueError."""
    try:
        fx, fy, cx, cy = (_f32(e) for e in K)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be (fx, fy, cx, cy) (got {K!r})") from None
    if not (all(math.isfinite(e) for e in (fx, fy, cx, cy)) and fx > 0.0 and fy > 0.0):
        raise ValueError(f"{name} must be (fx, fy, cx, cy) with entries finite in float32 and fx, fy > 0 (got {K!r})")
    return fx, fy, cx, cy


def check_scalars(threshold, baseline):
    """(threshold, baseline) as the ABI receives them (float32): pixels >= 0 whose square is finite in float32 (the kernels compare
    against it: up to about 1.8e19), and a finite length > 0, or the ValueError."""
    try:
        t, b = _f32(threshold), _f32(baseline)
    except (TypeError, ValueError):
        t = b = math.nan
    if not (t >= 0.0 and math.isfinite(_f32(t * t))):
        raise ValueError(f"threshold must be a number of pixels >= 0 whose square is finite in float32 (got {threshold!r})")
    if not (b > 0.0 and math.isfinite(b)):
        raise ValueError(f"baseline must be a length > 0, finite in float32 (got {baseline!r})")
    return t, b


def two_view_pose_args(ctx, ref_uv, cur_uv, status, K, K_cur, threshold: float, baseline: float, workspace, pose, points, E, n_front, valid, n_points,
                       stream=None):
    """Checks one ftk_two_view_pose_device call and returns its marshalled arguments."""
    from . import device as D

    cam = check_camera("K", K)
    cam_cur = cam if K_cur is None else check_camera("K_cur", K_cur)
    t, b = check_scalars(threshold, baseline)
    dev = D._call_device(ctx, ref_uv)
    D._check("ref_uv", ref_uv, D._F32, (None, 2), dev)
    n = int(ref_uv.shape[0])
    if not 1 <= n <= N.FTK_TRACK_TABLE_MAX_SLOTS:
        raise ValueError(f"ref_uv must have 1 .. FTK_TRACK_TABLE_MAX_SLOTS = {N.FTK_TRACK_TABLE_MAX_SLOTS} points (got {n})")
    D._check("cur_uv", cur_uv, D._F32, (n, 2), dev)
    D._check("status", status, D._U8, (n,), dev)
    D._check("workspace", workspace, D._KEYS, (None,), dev, min_numel=-(-N.two_view_pose_workspace_bytes(n) // 8))
    D._check("pose", pose, D._F32, (7,), dev)
    D._check("points", points, D._F32, (n, 3), dev)
    D._check("E", E, D._F32, (3, 3), dev)
    D._check("n_front", n_front, D._I32, (4,), dev)
    D._check("valid", valid, D._I32, (1,), dev)
    D._check("n_points", n_points, D._I32, (1,), dev)
    s = stream_or_current(ref_uv, stream)
    return ((ctx.handle, C.c_void_p(s.cuda_stream), pointer(ref_uv), pointer(cur_uv), pointer(status), n) + tuple(C.c_float(e) for e in cam + cam_cur)
            + (C.c_float(t), C.c_float(b), pointer(workspace), pointer(pose), pointer(points), pointer(E), pointer(n_front), pointer(valid), pointer(n_points)))


def two_view_pose_device(ctx, ref_uv, cur_uv, status, K, K_cur, threshold: float, baseline: float, workspace, pose, points, E, n_front, valid, n_points,
                         stream=None) -> None:
    """ftk_two_view_pose_device: the relative pose of two views and the landmarks of the correspondences ``ref_uv[i] -> cur_uv[i]``
    (contiguous float32 CUDA [n, 2], (u, v) pixels) whose ``status`` (uint8 [n]) is TRACKED, by the contract of DESIGN.md 5.29: the
    eight-point refit on all participants in a fixed summation tree, the essential projection, the cheirality vote and the two-ray
    triangulation.  ``K`` / ``K_cur``: (fx, fy, cx, cy) of the reference and the current view (``K_cur`` None: the same camera).
    ``pose`` float32 [7] receives q_rc (w, x, y, z) and p_rc in DirectMethod's convention with ``|p_rc| = baseline``, ``points`` float32
    [n, 3] the landmarks in the reference camera frame (zeros where there is none), ``E`` float32 [3, 3], ``n_front`` int32 [4],
    ``valid`` int32 [1] (1 / -1), ``n_points`` int32 [1]; ``status`` is rewritten in place (a participant without a landmark becomes
    LARGE_RESIDUAL; nothing changes when the result is invalid).  ``workspace``: int64 or uint64 CUDA tensor of at least
    ``_native.two_view_pose_workspace_bytes(n) / 8`` elements, no initialisation needed.  Five launches on ``stream`` (default: torch's
    current stream), no synchronisation, no allocation: capturable.  Every argument is checked before the device is touched."""
    args = two_view_pose_args(ctx, ref_uv, cur_uv, status, K, K_cur, threshold, baseline, workspace, pose, points, E, n_front, valid, n_points, stream)
    N.check(N.lib().ftk_two_view_pose_device(*args), ctx.handle)
