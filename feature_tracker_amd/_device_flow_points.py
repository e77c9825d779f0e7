"""``device.flow_track_points_device``: the torch device entry of sparse tracking from RAFT's coarse flow (ftk_flow_track_points_device,
DESIGN.md 5.17).

It is re-exported by device.py and held to that module's rule: no ``data_ptr()`` of a tensor that did not pass ``device._check``.
It lives in a file of its own because tests/test_device_args_cpu.py walks the entries DEFINED in device.py against a closed table;
this entry's walk (the same recording stand-ins) and its refusals are tests/test_flow_points_cpu.py.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _native as N
from ._torch_call import pointer, stream_or_current


def flow_track_points_device(ctx, flow, mask, points, image_rows: int, image_cols: int, cur_points, status, fb_error2=None, mask_scale: float = 1.0,
                             flow_back=None, mask_back=None, fb_threshold: float = 0.0, stream=None) -> None:
    """ftk_flow_track_points_device: ``points`` (contiguous float32 CUDA [B, N, 2], u = x and v = y in image pixels) tracked through the
    flow ``Raft.UpsampleFlow(flow, mask_scale * mask)`` (model.py:48-64) would give, of ``flow`` [B, 2, H, W] and ``mask`` [B, 576, H, W],
    in an image of ``image_rows`` x ``image_cols`` (at most 8H x 8W), into ``cur_points`` [B, N, 2], ``status`` (uint8 [B, N], TrackStatus)
    and, when given, ``fb_error2`` (float32 [B, N]).  ``flow_back`` and ``mask_back`` (both or neither, shaped like the forward pair) add
    the forward-backward check against ``fb_threshold`` pixels.  Enqueued on ``stream`` (a torch.cuda.Stream; default: torch's current
    stream).  One launch (none for N = 0), no synchronisation, no allocation: capturable.  Every argument is checked before the device
    is touched."""
    from . import device as D

    scale, threshold = float(mask_scale), float(fb_threshold)
    if not math.isfinite(scale):
        raise ValueError(f"mask_scale must be finite (got {mask_scale})")
    if not threshold >= 0:
        raise ValueError(f"fb_threshold must be a number >= 0 (got {fb_threshold})")
    if (flow_back is None) != (mask_back is None):
        raise ValueError(f"flow_back and mask_back go together (got {'flow_back' if mask_back is None else 'mask_back'} alone)")
    dev = D._call_device(ctx, flow)
    D._check("flow", flow, D._F32, (None, 2, None, None), dev)
    B, _, H, W = (int(e) for e in flow.shape)
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"flow must be a non-empty [B, 2, H, W] tensor (got {list(flow.shape)})")
    rows, cols = int(image_rows), int(image_cols)
    if not (1 <= rows <= 8 * H and 1 <= cols <= 8 * W):
        raise ValueError(f"image_rows x image_cols = {image_rows} x {image_cols} must be within 1 .. {8 * H} x 1 .. {8 * W}, the grid of the flow")
    D._check("mask", mask, D._F32, (B, 576, H, W), dev)
    D._check("points", points, D._F32, (B, None, 2), dev)
    n = int(points.shape[1])
    D._check("cur_points", cur_points, D._F32, (B, n, 2), dev)
    D._check("status", status, D._U8, (B, n), dev)
    if fb_error2 is not None:
        D._check("fb_error2", fb_error2, D._F32, (B, n), dev)
    if flow_back is not None:
        D._check("flow_back", flow_back, D._F32, (B, 2, H, W), dev)
        D._check("mask_back", mask_back, D._F32, (B, 576, H, W), dev)
    s = stream_or_current(flow, stream)
    rc = N.lib().ftk_flow_track_points_device(ctx.handle, C.c_void_p(s.cuda_stream), pointer(flow), pointer(mask), pointer(flow_back), pointer(mask_back), B, H, W, n,
                                              rows, cols, scale, threshold, pointer(points), pointer(cur_points), pointer(status), pointer(fb_error2))
    N.check(rc, ctx.handle)
