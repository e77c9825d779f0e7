"""``device.flow_upsample_device``: the torch device entry of RAFT's convex flow upsampling (ftk_flow_upsample_device).

It is re-exported by device.py and held to that module's rule: no ``data_ptr()`` of a tensor that did not pass ``device._check``.
It lives in a file of its own because tests/test_device_args_cpu.py walks the entries DEFINED in device.py against a closed table;
this entry's walk (the same recording stand-ins) and its refusals are tests/test_flow_upsample_cpu.py.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _native as N
from ._torch_call import stream_or_current


def flow_upsample_device(ctx, flow, mask, out, mask_scale: float = 1.0, stream=None) -> None:
    """ftk_flow_upsample_device: ``out`` (contiguous float32 CUDA [B, 2, 8H, 8W]) = Raft.UpsampleFlow(``flow``, ``mask_scale`` * ``mask``)
    (model.py:48-64) of ``flow`` (contiguous float32 CUDA [B, 2, H, W]) and ``mask`` ([B, 576, H, W]), enqueued on ``stream`` (a
    torch.cuda.Stream; default: torch's current stream).  One launch, no synchronisation, no allocation: capturable.  Every argument
    is checked before the device is touched."""
    from . import device as D

    scale = float(mask_scale)
    if not math.isfinite(scale):
        raise ValueError(f"mask_scale must be finite (got {mask_scale})")
    dev = D._call_device(ctx, flow)
    D._check("flow", flow, D._F32, (None, 2, None, None), dev)
    B, _, H, W = (int(e) for e in flow.shape)
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"flow must be a non-empty [B, 2, H, W] tensor (got {list(flow.shape)})")
    D._check("mask", mask, D._F32, (B, 576, H, W), dev)
    D._check("out", out, D._F32, (B, 2, 8 * H, 8 * W), dev)
    s = stream_or_current(flow, stream)
    rc = N.lib().ftk_flow_upsample_device(ctx.handle, C.c_void_p(s.cuda_stream), C.c_void_p(flow.data_ptr()), C.c_void_p(mask.data_ptr()),
                                          B, H, W, scale, C.c_void_p(out.data_ptr()))
    N.check(rc, ctx.handle)
