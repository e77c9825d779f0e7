"""``device.landmark_table_begin_device`` / ``device.landmark_table_end_device``: the torch device entries of the landmark table beside a
track table (ftk_landmark_table_begin_device, ftk_landmark_table_end_device).

They are re-exported by device.py and held to that module's rule: no ``datapointer()`` of a tensor that did not pass ``device._check``.  They
live in a file of their own for _device_epipolar.py's reason; their walk and their refusals are tests/test_track_odometry_args_cpu.py.
``TrackOdometry`` keeps the marshalled arguments, as ``KltVideoTracker`` keeps its own: its tensors are fixed.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _native as N
from ._device_klt_video import _I64
from ._device_two_view_pose import _f32, check_camera, check_scalars
from ._torch_call import pointer, stream_or_current

# where the per-call values stand in landmark_end_args' result (TrackOdometry replaces them in the list it keeps)
STREAM_ARG = 1  # of both entries
END_STATUS_ARG, END_POSE_ARG, END_VALID_ARG, END_MODEL_ARG, END_FRAME_ARG, END_MODE_ARG = 5, 6, 7, 8, 9, 10
_MAX_FRAME = 0x7FFFFFFF


def check_parallax(min_parallax_deg) -> float:
    """cos^2 of the parallax floor as the ABI receives it: float64 on the host, rounded to float32 once; 0 .. 90 degrees, or the ValueError."""
    try:
        deg = float(min_parallax_deg)
    except (TypeError, ValueError):
        deg = math.nan
    if not 0.0 <= deg <= 90.0:
        raise ValueError(f"min_parallax_deg must be an angle in 0 .. 90 degrees (got {min_parallax_deg!r})")
    c = math.cos(math.radians(deg))
    return _f32(c * c)


def check_frame_mode(frame, mode):
    try:
        f, m = int(frame), int(mode)
    except (TypeError, ValueError):
        raise ValueError(f"frame and mode must be integers (got {frame!r}, {mode!r})") from None
    if not 0 <= f <= _MAX_FRAME:
        raise ValueError(f"frame must be in 0 .. {_MAX_FRAME}: a negative anchor_frame means no anchor (got {frame})")
    if m not in (N.FTK_LANDMARK_TABLE_STEADY, N.FTK_LANDMARK_TABLE_BOOTSTRAP):
        raise ValueError(f"mode must be FTK_LANDMARK_TABLE_STEADY = 0 or FTK_LANDMARK_TABLE_BOOTSTRAP = 1 (got {mode})")
    return f, m


def _check_ids(D, ctx, ids):
    dev = D._call_device(ctx, ids)
    D._check("ids", ids, _I64, (None,), dev)
    n = int(ids.shape[0])
    if not 1 <= n <= N.FTK_TRACK_TABLE_MAX_SLOTS:
        raise ValueError(f"ids must have 1 .. FTK_TRACK_TABLE_MAX_SLOTS = {N.FTK_TRACK_TABLE_MAX_SLOTS} slots (got {n})")
    return n, dev


def landmark_begin_args(ctx, ids, owner, landmarks, anchor_frame, pnp_status, anchor_status, counters, stream=None):
    """Checks one ftk_landmark_table_begin_device call and returns its marshalled arguments."""
    from . import device as D

    n, dev = _check_ids(D, ctx, ids)
    D._check("owner", owner, _I64, (n,), dev)
    D._check("landmarks", landmarks, D._F32, (n, 3), dev)
    D._check("anchor_frame", anchor_frame, D._I32, (n,), dev)
    D._check("pnp_status", pnp_status, D._U8, (n,), dev)
    D._check("anchor_status", anchor_status, D._U8, (n,), dev)
    D._check("counters", counters, D._I32, (N.FTK_LANDMARK_TABLE_COUNTERS,), dev)
    st = stream_or_current(ids, stream)
    p = pointer
    return (ctx.handle, C.c_void_p(st.cuda_stream), p(ids), n, p(owner), p(landmarks), p(anchor_frame), p(pnp_status), p(anchor_status), p(counters))


def landmark_table_begin_device(ctx, ids, owner, landmarks, anchor_frame, pnp_status, anchor_status, counters, stream=None) -> None:
    """ftk_landmark_table_begin_device: a frame of the landmark table before its pose is known.  ``ids`` int64 CUDA [n] is the track table's;
    ``owner`` int64 [n], ``landmarks`` float32 [n, 3] and ``anchor_frame`` int32 [n] are the table's state: a slot whose id is not its
    owner's gets the new owner, a zero landmark and no anchor.  ``pnp_status`` / ``anchor_status`` uint8 [n] receive TRACKED for a live slot
    with a landmark / with an anchor and NOT_TRACKED otherwise; ``counters`` int32 [FTK_LANDMARK_TABLE_COUNTERS]: the four that the end
    entry adds to are zeroed.  One launch on ``stream`` (default: torch's current stream), nothing read back: capturable."""
    N.check(N.lib().ftk_landmark_table_begin_device(*landmark_begin_args(ctx, ids, owner, landmarks, anchor_frame, pnp_status, anchor_status, counters, stream)),
            ctx.handle)


def landmark_end_args(ctx, ids, points, status_in, pose_in, valid_in, model_in, frame: int, mode: int, K, threshold: float, min_parallax_cos2: float,
                      landmarks, anchor_uv, anchor_pose, anchor_frame, counters, pose, stream=None):
    """Checks one ftk_landmark_table_end_device call and returns its marshalled arguments."""
    from . import device as D

    cam = check_camera("K", K)
    t, _ = check_scalars(threshold, 1.0)
    f, m = check_frame_mode(frame, mode)
    try:
        c2 = _f32(min_parallax_cos2)
    except (TypeError, ValueError):
        c2 = math.nan
    if not 0.0 <= c2 <= 1.0:
        raise ValueError(f"min_parallax_cos2 must be a squared cosine in 0 .. 1 (got {min_parallax_cos2!r})")
    if status_in is None and m == N.FTK_LANDMARK_TABLE_STEADY:
        raise ValueError("status_in must be given in steady mode: rule a reads it")
    n, dev = _check_ids(D, ctx, ids)
    D._check("points", points, D._F32, (n, 2), dev)
    if status_in is not None:
        D._check("status_in", status_in, D._U8, (n,), dev)
    D._check("pose_in", pose_in, D._F32, (7,), dev)
    D._check("valid_in", valid_in, D._I32, (1,), dev)
    if model_in is not None:
        D._check("model_in", model_in, D._I32, (1,), dev)
    D._check("landmarks", landmarks, D._F32, (n, 3), dev)
    D._check("anchor_uv", anchor_uv, D._F32, (n, 2), dev)
    D._check("anchor_pose", anchor_pose, D._F32, (n, 7), dev)
    D._check("anchor_frame", anchor_frame, D._I32, (n,), dev)
    D._check("counters", counters, D._I32, (N.FTK_LANDMARK_TABLE_COUNTERS,), dev)
    D._check("pose", pose, D._F32, (7,), dev)
    st = stream_or_current(ids, stream)
    p = pointer
    return ((ctx.handle, C.c_void_p(st.cuda_stream), p(ids), p(points), n, p(status_in), p(pose_in), p(valid_in), p(model_in), f, m)
            + tuple(C.c_float(e) for e in cam) + (C.c_float(t), C.c_float(c2), p(landmarks), p(anchor_uv), p(anchor_pose), p(anchor_frame), p(counters), p(pose)))


def landmark_table_end_device(ctx, ids, points, status_in, pose_in, valid_in, model_in, frame: int, mode: int, K, threshold: float,
                              min_parallax_cos2: float, landmarks, anchor_uv, anchor_pose, anchor_frame, counters, pose, stream=None) -> None:
    """ftk_landmark_table_end_device: a frame of the landmark table after its pose is known, by the contract of DESIGN.md 5.31.  ``ids`` /
    ``points`` (int64 [n], float32 [n, 2]): the track table; ``pose_in`` float32 [7] / ``valid_in`` int32 [1]: this frame's pose and its
    validity (``PnpRansac``'s outputs, ``TwoViewPose``'s in the bootstrap); ``model_in`` int32 [1] or None: ``TwoViewRansac``'s choice, a
    homography counts as invalid; ``status_in`` uint8 [n]: the status ``PnpRansac`` left (None in bootstrap mode).  ``mode``:
    FTK_LANDMARK_TABLE_STEADY or FTK_LANDMARK_TABLE_BOOTSTRAP.  ``K``: (fx, fy, cx, cy); ``min_parallax_cos2``: see ``check_parallax``.
    ``landmarks`` [n, 3], ``anchor_uv`` [n, 2], ``anchor_pose`` [n, 7], ``anchor_frame`` [n], ``counters`` [FTK_LANDMARK_TABLE_COUNTERS]
    and ``pose`` [7] are rewritten in place.  One launch on ``stream`` (default: torch's current stream), nothing read back: capturable.
    Every argument is checked before the device is touched."""
    args = landmark_end_args(ctx, ids, points, status_in, pose_in, valid_in, model_in, frame, mode, K, threshold, min_parallax_cos2, landmarks, anchor_uv,
                             anchor_pose, anchor_frame, counters, pose, stream)
    N.check(N.lib().ftk_landmark_table_end_device(*args), ctx.handle)
