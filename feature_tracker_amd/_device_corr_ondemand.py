"""``device.corr_ondemand_prepare_device`` / ``device.corr_ondemand_lookup_device``: the torch device entries of RAFT's on-demand correlation
(ftk_corr_ondemand_*_device).

They are re-exported by device.py and held to that module's rule: no ``data_ptr()`` of a tensor that did not pass ``device._check``.
They live in a file of their own because tests/test_device_args_cpu.py walks the entries DEFINED in device.py against a closed table;
these entries' walk (the same recording stand-ins) and their refusals are tests/test_raft_corr_ondemand_cpu.py.
"""
from __future__ import annotations

import ctypes as C

from . import _native as N
from ._torch_call import stream_or_current


def corr_ondemand_prepare_device(ctx, fmap0, fmap1, levels: int, workspace, stream=None) -> None:
    """ftk_corr_ondemand_prepare_device: ``fmap0`` / ``fmap1`` (contiguous float32 CUDA [B, C, H, W]) transposed, and ``fmap1`` pooled through
    ``levels`` levels, into ``workspace`` (contiguous float32 CUDA, ftk_corr_ondemand_layout's element count), enqueued on ``stream`` (a
    torch.cuda.Stream; default: torch's current stream).  No synchronisation, no allocation: capturable."""
    from . import device as D

    D._torch()  # (no HIP device: that refusal comes first)
    D._corr_check("fmap0", fmap0, 4)
    D._corr_check("fmap1", fmap1, 4)
    if tuple(fmap0.shape) != tuple(fmap1.shape) or fmap0.device != fmap1.device:
        raise ValueError(f"fmap0 and fmap1 differ: {tuple(fmap0.shape)} on {fmap0.device} vs {tuple(fmap1.shape)} on {fmap1.device}")
    B, Cc, H, W = fmap0.shape
    elements, _, _ = N.corr_ondemand_layout(B, Cc, H, W, levels)
    D._corr_check("workspace", workspace, workspace.dim())
    if workspace.numel() != elements or workspace.device != fmap0.device:
        raise ValueError(f"workspace must hold {elements} floats on {fmap0.device} (got {workspace.numel()} on {workspace.device})")
    s = stream_or_current(fmap0, stream)
    rc = N.lib().ftk_corr_ondemand_prepare_device(ctx.handle, C.c_void_p(s.cuda_stream), C.c_void_p(fmap0.data_ptr()), C.c_void_p(fmap1.data_ptr()),
                                                  B, Cc, H, W, int(levels), C.c_void_p(workspace.data_ptr()))
    N.check(rc, ctx.handle)


def corr_ondemand_lookup_device(ctx, workspace, channels: int, levels: int, radius: int, coords, out, per_level: bool = False,
                                stream=None) -> None:
    """ftk_corr_ondemand_lookup_device: the (2r+1)^2 windows of every level around ``coords`` (contiguous float32 CUDA [B, 2, H, W], x then y)
    from a prepared ``workspace`` of ``channels`` channels into ``out``: [B, levels * K, H, W], or with ``per_level`` ``levels`` consecutive
    [B, H, W, K] blocks (K = (2r+1)^2)."""
    from . import device as D

    D._torch()  # (no HIP device: that refusal comes first)
    D._corr_check("coords", coords, 4)
    B, two, H, W = coords.shape
    if two != 2:
        raise ValueError(f"coords must be [B, 2, H, W] (got {tuple(coords.shape)})")
    elements, _, _ = N.corr_ondemand_layout(B, channels, H, W, levels)
    D._corr_check("workspace", workspace, workspace.dim())
    if workspace.numel() != elements or workspace.device != coords.device:
        raise ValueError(f"workspace must hold {elements} floats on {coords.device} (got {workspace.numel()} on {workspace.device})")
    if not 0 <= int(radius) <= N.FTK_CORR_MAX_RADIUS:
        raise ValueError(f"radius {radius} outside 0 .. {N.FTK_CORR_MAX_RADIUS}")
    K = (2 * int(radius) + 1) ** 2
    D._corr_check("out", out, out.dim())
    if out.numel() != B * levels * K * H * W or out.device != coords.device:
        raise ValueError(f"out must hold {B * levels * K * H * W} floats on {coords.device}")
    s = stream_or_current(coords, stream)
    rc = N.lib().ftk_corr_ondemand_lookup_device(ctx.handle, C.c_void_p(s.cuda_stream), C.c_void_p(workspace.data_ptr()), B, int(channels), H, W,
                                                 int(levels), int(radius), C.c_void_p(coords.data_ptr()), C.c_void_p(out.data_ptr()),
                                                 int(bool(per_level)))
    N.check(rc, ctx.handle)
