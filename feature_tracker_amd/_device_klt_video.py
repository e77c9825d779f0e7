"""``device.harris_detect_device`` and the two track-table entries: the torch device entries under ``KltVideoTracker``.

They are re-exported by device.py and held to that module's rule: no ``data_ptr()`` of a tensor that did not pass ``device._check``.
They live in a file of their own because tests/test_device_args_cpu.py walks the entries DEFINED in device.py against a closed table;
these entries' walk (the same recording stand-ins) and their refusals are tests/test_klt_video_args_cpu.py.
"""
from __future__ import annotations

import ctypes as C

from . import _native as N
from ._torch_call import pointer

_I64 = ("int64",)


def harris_survivor_bound(rows: int, cols: int, min_distance: int) -> int:
    """ceil(rows / d) * ceil(cols / d), d = max(min_distance, 1): survivors keep Chebyshev distance d, so no image holds more; 0 for an
    image below 23 x 23, which has no valid centre.  The device list is sized by it (csrc/track_table_plan.h)."""
    d = max(int(min_distance), 1)
    if int(rows) < 23 or int(cols) < 23:
        return 0
    return -(-int(rows) // d) * -(-int(cols) // d)


def _check_bound(rows, cols, min_distance):
    bound = harris_survivor_bound(rows, cols, min_distance)
    if bound > N.FTK_HARRIS_DEVICE_MAX_SURVIVORS:
        raise ValueError(f"a {rows} x {cols} image at min_distance {int(min_distance)} can hold {bound} corners, above "
                         f"FTK_HARRIS_DEVICE_MAX_SURVIVORS = {N.FTK_HARRIS_DEVICE_MAX_SURVIVORS}: raise min_distance")


def harris_detect_device(ctx, pyramid, max_count: int, min_distance: int, min_response: float, uv_out, count_out, occupied=None, occupied_mask=None,
                         level: int = 0) -> None:
    """ftk_harris_detect_device: Harris corners of level ``level`` of ``pyramid`` that keep their distance from the points that already exist,
    into ``uv_out`` (contiguous float32 CUDA [max_count, 2]: the strongest survivors as (col, row), zeros behind them) and ``count_out``
    (int32 CUDA [1]).  ``occupied``: float32 CUDA [n, 2] or None; ``occupied_mask``: uint8 CUDA [n] (a point counts where its byte is not 0)
    or None for all of them.  Enqueued on the context's stream; no copy to the host, no synchronisation.  Every argument is checked before
    the device is touched; a survivor bound above FTK_HARRIS_DEVICE_MAX_SURVIVORS is a ValueError."""
    from . import device as D

    k = int(max_count)
    if k < 0:
        raise ValueError(f"max_count must not be negative (got {max_count})")
    if occupied is None and occupied_mask is not None:
        raise ValueError("occupied_mask without occupied: the mask selects among the occupied points")
    _, rows, cols = pyramid.level_desc(int(level))
    _check_bound(rows, cols, min_distance)
    dev = D._call_device(ctx, uv_out)
    D._check("uv_out", uv_out, D._F32, (k, 2), dev)
    D._check("count_out", count_out, D._I32, (1,), dev)
    n = 0
    if occupied is not None:
        D._check("occupied", occupied, D._F32, (None, 2), dev)
        n = int(occupied.shape[0])
        if occupied_mask is not None:
            D._check("occupied_mask", occupied_mask, D._U8, (n,), dev)
    rc = N.lib().ftk_harris_detect_device(ctx.handle, pyramid.handle, int(level), k, int(min_distance), float(min_response),
                                          pointer(occupied), pointer(occupied_mask), n, pointer(uv_out), pointer(count_out))
    N.check(rc, ctx.handle)


def _check_table(D, ctx, ids, points, prev_points, status, age, n_live):
    """The table's tensors (include/ftk.h): ids int64 [n], points / prev_points float32 [n, 2], status uint8 [n], age int32 [n], n_live int32 [1]."""
    dev = D._call_device(ctx, ids)
    D._check("ids", ids, _I64, (None,), dev)
    n = int(ids.shape[0])
    if not 1 <= n <= N.FTK_TRACK_TABLE_MAX_SLOTS:
        raise ValueError(f"ids must have 1 .. {N.FTK_TRACK_TABLE_MAX_SLOTS} slots (got {n})")
    D._check("points", points, D._F32, (n, 2), dev)
    D._check("prev_points", prev_points, D._F32, (n, 2), dev)
    D._check("status", status, D._U8, (n,), dev)
    D._check("age", age, D._I32, (n,), dev)
    D._check("n_live", n_live, D._I32, (1,), dev)
    return n, dev


def track_table_retire_args(ctx, ids, points, prev_points, status, age, n_live, tracked_uv, tracked_status, free_slots, n_free, back_uv=None,
                            back_status=None, fb_threshold: float = 0.0):
    """Checks one ftk_track_table_retire_device call and returns its marshalled arguments (KltVideoTracker keeps them: its tensors are fixed)."""
    from . import device as D

    if (back_uv is None) != (back_status is None):
        raise ValueError("back_uv and back_status go together: the forward-backward check needs both")
    if back_uv is not None and not float(fb_threshold) >= 0.0:
        raise ValueError(f"fb_threshold must be >= 0 (got {fb_threshold})")
    n, dev = _check_table(D, ctx, ids, points, prev_points, status, age, n_live)
    D._check("tracked_uv", tracked_uv, D._F32, (n, 2), dev)
    D._check("tracked_status", tracked_status, D._U8, (n,), dev)
    if back_uv is not None:
        D._check("back_uv", back_uv, D._F32, (n, 2), dev)
        D._check("back_status", back_status, D._U8, (n,), dev)
    D._check("free_slots", free_slots, D._I32, (n,), dev)
    D._check("n_free", n_free, D._I32, (1,), dev)
    p = pointer
    return (ctx.handle, n, p(ids), p(points), p(prev_points), p(status), p(age), p(n_live), p(tracked_uv), p(tracked_status), p(back_uv), p(back_status),
            C.c_float(float(fb_threshold)), p(free_slots), p(n_free))


def track_table_retire_device(ctx, ids, points, prev_points, status, age, n_live, tracked_uv, tracked_status, free_slots, n_free, back_uv=None,
                              back_status=None, fb_threshold: float = 0.0) -> None:
    """ftk_track_table_retire_device: after a frame's tracker call(s) (``tracked_uv`` float32 [n, 2], ``tracked_status`` uint8 [n]; with the
    forward-backward check ``back_uv`` / ``back_status`` and ``fb_threshold``), the slots that stay live move on, the others are emptied,
    and ``free_slots`` (int32 [n]) lists every empty slot in ascending order, ``n_free`` (int32 [1]) their number.  One launch on the
    context's stream, nothing read back."""
    args = track_table_retire_args(ctx, ids, points, prev_points, status, age, n_live, tracked_uv, tracked_status, free_slots, n_free, back_uv, back_status,
                                   fb_threshold)
    N.check(N.lib().ftk_track_table_retire_device(*args), ctx.handle)


def track_table_fill_args(ctx, pyramid, min_distance: int, min_response: float, ids, points, prev_points, status, age, n_live, next_id, free_slots, n_free,
                          level: int = 0):
    """Checks one ftk_track_table_fill_device call and returns its marshalled arguments."""
    from . import device as D

    _, rows, cols = pyramid.level_desc(int(level))
    _check_bound(rows, cols, min_distance)
    n, dev = _check_table(D, ctx, ids, points, prev_points, status, age, n_live)
    D._check("next_id", next_id, _I64, (1,), dev)
    D._check("free_slots", free_slots, D._I32, (n,), dev)
    D._check("n_free", n_free, D._I32, (1,), dev)
    p = pointer
    return (ctx.handle, pyramid.handle, int(level), int(min_distance), C.c_float(float(min_response)), n, p(ids), p(points), p(prev_points), p(status), p(age),
            p(n_live), p(next_id), p(free_slots), p(n_free))


def track_table_fill_device(ctx, pyramid, min_distance: int, min_response: float, ids, points, prev_points, status, age, n_live, next_id, free_slots,
                            n_free, level: int = 0) -> None:
    """ftk_track_table_fill_device: masked Harris detection on ``pyramid`` with the live slots as occupied points, and the survivor of rank
    r < n_free into slot free_slots[r] with id next_id + r; next_id (int64 [1]) and n_live grow by the number filled.  On the context's
    stream, nothing read back."""
    args = track_table_fill_args(ctx, pyramid, min_distance, min_response, ids, points, prev_points, status, age, n_live, next_id, free_slots, n_free, level)
    N.check(N.lib().ftk_track_table_fill_device(*args), ctx.handle)
