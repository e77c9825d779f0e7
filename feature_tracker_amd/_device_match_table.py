"""``device.match_table_query_device`` and ``device.match_table_update_device``: the torch device entries under ``MatchVideoTracker``
(ftk_match_table_*_device).

They are re-exported by device.py and held to that module's rule: no ``data_ptr()`` of a tensor that did not pass ``device._check``.
They live in a file of their own for _device_klt_video.py's reason; their walk and their refusals are tests/test_match_table_args_cpu.py.
"""
from __future__ import annotations

import ctypes as C

from . import _native as N
from ._torch_call import pointer, stream_or_current

_I64 = ("int64",)


def check_sizes(n_slots: int, rows_cur: int, dim: int) -> None:
    """The limits of include/ftk.h."""
    if not 1 <= n_slots <= N.FTK_MATCH_TABLE_MAX_SLOTS:
        raise ValueError(f"ids must have 1 .. FTK_MATCH_TABLE_MAX_SLOTS = {N.FTK_MATCH_TABLE_MAX_SLOTS} slots (got {n_slots})")
    if not 1 <= rows_cur <= N.FTK_MATCH_TABLE_MAX_SLOTS:
        raise ValueError(f"cur_uv must have 1 .. FTK_MATCH_TABLE_MAX_SLOTS = {N.FTK_MATCH_TABLE_MAX_SLOTS} rows (got {rows_cur})")
    if not 1 <= dim <= N.FTK_MATCH_TABLE_MAX_DIM:
        raise ValueError(f"descriptors must have 1 .. FTK_MATCH_TABLE_MAX_DIM = {N.FTK_MATCH_TABLE_MAX_DIM} columns (got {dim})")


def check_max_lost(max_lost) -> int:
    """``max_lost`` as the ABI takes it, or the ValueError."""
    if isinstance(max_lost, bool) or not isinstance(max_lost, int) or not 0 <= max_lost < 1 << 31:
        raise ValueError(f"max_lost must be an integer >= 0 (got {max_lost!r})")
    return max_lost


def _refuse_aliases(named) -> None:
    """No argument may alias another: two names for one tensor object are refused here, equal pointers by the library."""
    seen = {}
    for name, t in named:
        if t is None:
            continue
        if id(t) in seen:
            raise ValueError(f"{name} and {seen[id(t)]} are one tensor: no argument may alias another")
        seen[id(t)] = name


def match_table_query_args(ctx, ids, points, descriptors, q_uv, q_desc, q_slot, q_count, stream=None):
    """Checks one ftk_match_table_query_device call and returns its marshalled arguments (MatchVideoTracker keeps them: its tensors are fixed)."""
    from . import device as D

    _refuse_aliases((("ids", ids), ("points", points), ("descriptors", descriptors), ("q_uv", q_uv), ("q_desc", q_desc), ("q_slot", q_slot),
                     ("q_count", q_count)))
    dev = D._call_device(ctx, ids)
    D._check("ids", ids, _I64, (None,), dev)
    n = int(ids.shape[0])
    D._check("descriptors", descriptors, D._F32, (n, None), dev)
    d = int(descriptors.shape[1])
    check_sizes(n, 1, d)
    D._check("points", points, D._F32, (n, 2), dev)
    D._check("q_uv", q_uv, D._F32, (n, 2), dev)
    D._check("q_desc", q_desc, D._F32, (n, d), dev)
    D._check("q_slot", q_slot, D._I32, (n,), dev)
    D._check("q_count", q_count, D._I32, (1,), dev)
    st = stream_or_current(ids, stream)
    p = pointer
    return (ctx.handle, C.c_void_p(st.cuda_stream), n, d, p(ids), p(points), p(descriptors), p(q_uv), p(q_desc), p(q_slot), p(q_count))


def match_table_query_device(ctx, ids, points, descriptors, q_uv, q_desc, q_slot, q_count, stream=None) -> None:
    """ftk_match_table_query_device: the live slots of the table (``ids`` int64 [n], ``points`` float32 [n, 2], ``descriptors`` float32
    [n, D], contiguous CUDA tensors) in ascending slot order as rows 0 .. nq - 1 of ``q_uv`` [n, 2], ``q_desc`` [n, D] and ``q_slot``
    int32 [n]; ``q_count`` int32 [1] = nq; rows behind it are +0 and -1.  2 launches on ``stream`` (default: torch's current stream), no
    synchronisation, no allocation: capturable.  Every argument is checked before the device is touched."""
    args = match_table_query_args(ctx, ids, points, descriptors, q_uv, q_desc, q_slot, q_count, stream)
    N.check(N.lib().ftk_match_table_query_device(*args), ctx.handle)


def match_table_update_args(ctx, ids, points, prev_points, descriptors, status, age, lost, n_live, next_id, q_slot, q_count, match_index, match_status,
                            cur_uv, cur_desc, cur_count, max_lost, workspace, cur_slot=None, stream=None):
    """Checks one ftk_match_table_update_device call and returns its marshalled arguments."""
    from . import device as D

    lost_frames = check_max_lost(max_lost)
    _refuse_aliases((("ids", ids), ("points", points), ("prev_points", prev_points), ("descriptors", descriptors), ("status", status), ("age", age),
                     ("lost", lost), ("n_live", n_live), ("next_id", next_id), ("q_slot", q_slot), ("q_count", q_count), ("match_index", match_index),
                     ("match_status", match_status), ("cur_uv", cur_uv), ("cur_desc", cur_desc), ("cur_count", cur_count), ("workspace", workspace),
                     ("cur_slot", cur_slot)))
    dev = D._call_device(ctx, ids)
    D._check("ids", ids, _I64, (None,), dev)
    n = int(ids.shape[0])
    D._check("descriptors", descriptors, D._F32, (n, None), dev)
    d = int(descriptors.shape[1])
    D._check("cur_uv", cur_uv, D._F32, (None, 2), dev)
    k = int(cur_uv.shape[0])
    check_sizes(n, k, d)
    D._check("points", points, D._F32, (n, 2), dev)
    D._check("prev_points", prev_points, D._F32, (n, 2), dev)
    D._check("status", status, D._U8, (n,), dev)
    D._check("age", age, D._I32, (n,), dev)
    D._check("lost", lost, D._I32, (n,), dev)
    D._check("n_live", n_live, D._I32, (1,), dev)
    D._check("next_id", next_id, _I64, (1,), dev)
    D._check("q_slot", q_slot, D._I32, (n,), dev)
    D._check("q_count", q_count, D._I32, (1,), dev)
    D._check("match_index", match_index, D._I32, (n,), dev)
    D._check("match_status", match_status, D._U8, (n,), dev)
    D._check("cur_desc", cur_desc, D._F32, (k, d), dev)
    if cur_count is not None:
        D._check("cur_count", cur_count, D._I32, (1,), dev)
    D._check("workspace", workspace, D._KEYS, (None,), dev, min_numel=-(-N.match_table_workspace_bytes(n, k, d) // 8))
    if cur_slot is not None:
        D._check("cur_slot", cur_slot, D._I32, (k,), dev)
    st = stream_or_current(ids, stream)
    p = pointer
    return (ctx.handle, C.c_void_p(st.cuda_stream), n, d, p(ids), p(points), p(prev_points), p(descriptors), p(status), p(age), p(lost), p(n_live), p(next_id),
            p(q_slot), p(q_count), p(match_index), p(match_status), p(cur_uv), p(cur_desc), k, p(cur_count), lost_frames, p(workspace), p(cur_slot))


def match_table_update_device(ctx, ids, points, prev_points, descriptors, status, age, lost, n_live, next_id, q_slot, q_count, match_index, match_status,
                              cur_uv, cur_desc, cur_count, max_lost, workspace, cur_slot=None, stream=None) -> None:
    """ftk_match_table_update_device: one frame's matches (``match_index`` int32 [n], ``match_status`` uint8 [n], for the query rows
    ``q_slot`` / ``q_count`` against ``cur_uv`` float32 [K, 2] and ``cur_desc`` [K, D]; ``cur_count`` int32 [1] or None) into the table:
    hits move on, misses age and retire once ``lost > max_lost``, and the current rows no query row named fill the empty slots in order
    with ids from ``next_id`` (include/ftk.h states the contract).  ``workspace``: int64 or uint64 CUDA tensor of at least
    ``_native.match_table_workspace_bytes(n, K, D) / 8`` elements; ``cur_slot``: int32 [K] or None.  2 launches on ``stream``, no
    synchronisation, no allocation: capturable.  Every argument is checked before the device is touched."""
    args = match_table_update_args(ctx, ids, points, prev_points, descriptors, status, age, lost, n_live, next_id, q_slot, q_count, match_index, match_status,
                                   cur_uv, cur_desc, cur_count, max_lost, workspace, cur_slot, stream)
    N.check(N.lib().ftk_match_table_update_device(*args), ctx.handle)
