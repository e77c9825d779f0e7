"""``device.match_assignment_device``: the torch device entry of LightGlue's assignment head (ftk_match_assignment_device).

It is re-exported by device.py and held to that module's rule: no ``data_ptr()`` of a tensor that did not pass ``device._check``.  It lives
in a file of its own for _device_klt_video.py's reason; its walk and its refusals are tests/test_match_assignment_args_cpu.py.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _native as N
from ._torch_call import pointer, stream_or_current


def check_scale(scale) -> float:
    """``scale`` as the ABI takes it, or the ValueError."""
    try:
        s = float(scale)
    except (TypeError, ValueError):
        s = math.nan
    if isinstance(scale, bool) or not math.isfinite(s) or not 0.0 < s <= 3.0e38:
        raise ValueError(f"scale must be a finite number > 0 (got {scale!r})")
    return s


def check_sizes(rows0: int, rows1: int, dim: int) -> None:
    """The limits of include/ftk.h."""
    if not (1 <= rows0 <= N.FTK_MATCH_ASSIGNMENT_MAX_ROWS and 1 <= rows1 <= N.FTK_MATCH_ASSIGNMENT_MAX_ROWS):
        raise ValueError(f"desc0 and desc1 must have 1 .. FTK_MATCH_ASSIGNMENT_MAX_ROWS = {N.FTK_MATCH_ASSIGNMENT_MAX_ROWS} rows (got {rows0} and {rows1})")
    if not 1 <= dim <= N.FTK_MATCH_ASSIGNMENT_MAX_DIM:
        raise ValueError(f"descriptors must have 1 .. FTK_MATCH_ASSIGNMENT_MAX_DIM = {N.FTK_MATCH_ASSIGNMENT_MAX_DIM} columns (got {dim})")


def check_row_stride(row_stride, rows1: int) -> int:
    """``row_stride`` (None: rows1 + 1) in floats, or the ValueError."""
    if row_stride is None:
        return rows1 + 1
    if isinstance(row_stride, bool) or not isinstance(row_stride, int):
        raise ValueError(f"row_stride must be an integer (got {row_stride!r})")
    if not rows1 + 1 <= row_stride <= 1 << 24:
        raise ValueError(f"row_stride must be at least N + 1 = {rows1 + 1} and at most 2^24 (got {row_stride})")
    return row_stride


def match_assignment_args(ctx, desc0, desc1, weights, bias, scale, count0, count1, workspace, scores, row_stride=None, stream=None):
    """Checks one ftk_match_assignment_device call and returns its marshalled arguments."""
    from . import device as D

    if (weights is None) != (bias is None):
        raise ValueError(f"weights and bias go together (got {'weights' if bias is None else 'bias'} alone)")
    s = 1.0 if weights is not None else check_scale(scale)
    dev = D._call_device(ctx, desc0)
    D._check("desc0", desc0, D._F32, (None, None), dev)
    m, d = int(desc0.shape[0]), int(desc0.shape[1])
    D._check("desc1", desc1, D._F32, (None, d), dev)
    n = int(desc1.shape[0])
    check_sizes(m, n, d)
    if weights is not None:
        D._check("weights", weights, D._F32, (d + 1, d), dev)
        D._check("bias", bias, D._F32, (d + 1,), dev)
    if count0 is not None:
        D._check("count0", count0, D._I32, (1,), dev)
    if count1 is not None:
        D._check("count1", count1, D._I32, (1,), dev)
    stride = check_row_stride(row_stride, n)
    D._check("workspace", workspace, D._KEYS, (None,), dev, min_numel=-(-N.match_assignment_workspace_bytes(m, n, d, weights is not None) // 8))
    D._check("scores", scores, D._F32, (None,), dev, min_numel=m * stride + n + 1)
    st = stream_or_current(desc0, stream)
    p = pointer
    return (ctx.handle, C.c_void_p(st.cuda_stream), p(desc0), m, p(desc1), n, d, p(weights), p(bias), C.c_float(s), p(count0), p(count1), p(workspace),
            p(scores), stride)


def match_assignment_device(ctx, desc0, desc1, weights, bias, scale, count0, count1, workspace, scores, row_stride=None, stream=None) -> None:
    """ftk_match_assignment_device: descriptors ``desc0`` (contiguous float32 CUDA [M, D]) and ``desc1`` ([N, D]) to LightGlue's
    log-assignment tensor in ``scores``, a flat float32 buffer of at least ``M * row_stride + N + 1`` elements holding M + 1 rows of
    ``row_stride`` floats (default N + 1), of which the first N + 1 are written.  ``weights`` float32 [D + 1, D] (final_proj.weight, then
    matchability.weight) and ``bias`` float32 [D + 1], or both None: the descriptors as they are, times ``scale``.  ``count0`` / ``count1``:
    int32 [1] device tensors or None.  ``workspace``: int64 or uint64 CUDA tensor of at least
    ``_native.match_assignment_workspace_bytes(M, N, D, with_weights) / 8`` elements.  4 launches (3 without weights) on ``stream``
    (default: torch's current stream), no synchronisation, no allocation: capturable.  Every argument is checked before the device is
    touched."""
    args = match_assignment_args(ctx, desc0, desc1, weights, bias, scale, count0, count1, workspace, scores, row_stride, stream)
    N.check(N.lib().ftk_match_assignment_device(*args), ctx.handle)
