"""``device.flow_warm_device``: the torch device entry of the warm start of RAFT on video (ftk_flow_warm_device).

It is re-exported by device.py and held to that module's rule: no ``data_ptr()`` of a tensor that did not pass ``device._check``.
It lives in a file of its own because tests/test_device_args_cpu.py walks the entries DEFINED in device.py against a closed table;
this entry's walk (the same recording stand-ins) and its refusals are tests/test_flow_warm_args_cpu.py.
"""
from __future__ import annotations

import ctypes as C

from . import _native as N
from ._torch_call import stream_or_current


def flow_warm_device(ctx, flow, out, splits: int = 1, workspace=None, stream=None) -> None:
    """ftk_flow_warm_device: ``out`` (contiguous float32 CUDA [B, 2, H, W], not ``flow`` itself) = ``flow`` (the same) pushed forward along itself, what
    upstream RAFT's ``forward_interpolate`` computes on the host.  ``splits`` ranges of the sources are scanned by as many times the
    workgroups (``_native.flow_warm_splits`` gives the count that fills the chip; the result does not depend on it); above 1,
    ``workspace`` is a contiguous int64 or uint64 CUDA tensor of at least ``splits * B * H * W`` elements, which needs no initialisation.
    Enqueued on ``stream`` (a torch.cuda.Stream; default: torch's current stream).  One launch, two with ``splits`` above 1, no
    synchronisation, no allocation: capturable.  Every argument is checked before the device is touched."""
    from . import device as D

    k = int(splits)
    if not 1 <= k <= N.FTK_FLOW_WARM_MAX_SPLITS:
        raise ValueError(f"splits must be in 1 .. {N.FTK_FLOW_WARM_MAX_SPLITS} (got {splits})")
    if (k > 1) != (workspace is not None):
        raise ValueError(f"splits above 1 and workspace go together (got splits {k} {'without' if workspace is None else 'with'} a workspace)")
    dev = D._call_device(ctx, flow)
    D._check("flow", flow, D._F32, (None, 2, None, None), dev)
    B, _, H, W = (int(e) for e in flow.shape)
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"flow must be a non-empty [B, 2, H, W] tensor (got {list(flow.shape)})")
    if H * W > N.FTK_FLOW_WARM_MAX_PIXELS:
        raise ValueError(f"flow of {H} x {W} pixels is above FTK_FLOW_WARM_MAX_PIXELS = {N.FTK_FLOW_WARM_MAX_PIXELS}: the search is exhaustive")
    D._check("out", out, D._F32, (B, 2, H, W), dev)
    if workspace is not None:
        D._check("workspace", workspace, D._KEYS, (None,), dev, min_numel=k * B * H * W)
    s = stream_or_current(flow, stream)
    rc = N.lib().ftk_flow_warm_device(ctx.handle, C.c_void_p(s.cuda_stream), C.c_void_p(flow.data_ptr()), B, H, W, k,
                                      None if workspace is None else C.c_void_p(workspace.data_ptr()), C.c_void_p(out.data_ptr()))
    N.check(rc, ctx.handle)
