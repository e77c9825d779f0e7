"""``device.sep_conv_gru_device``: the torch device entry of RAFT's separable ConvGRU (ftk_sep_conv_gru_*_device).

It is re-exported by device.py and held to that module's rule: no ``data_ptr()`` of a tensor that did not pass ``device._check``.
It lives in a file of its own because tests/test_device_args_cpu.py walks the entries DEFINED in device.py against a closed table;
this entry's walk (the same recording stand-ins) and its refusals are tests/test_sep_conv_gru_cpu.py.
"""
from __future__ import annotations

import ctypes as C

from . import _native as N
from ._torch_call import stream_or_current

# the packed tensors a call needs, per pass: the stacked z | r matrix and bias, the q matrix and bias
PACKED_KEYS = ("zr_horizontal", "zr_bias_horizontal", "q_horizontal", "q_bias_horizontal",
               "zr_vertical", "zr_bias_vertical", "q_vertical", "q_bias_vertical")


def sep_conv_gru_device(ctx, x_parts, h, packed, kernel_size: int, z, rh, mid, out, stream=None) -> None:
    """SepConvGru.forward (gru.py:59-76) in four launches on ``stream`` (a torch.cuda.Stream; default: torch's current stream): gates
    and candidate + blend of the horizontal pass (``h`` -> ``mid``), then of the vertical pass (``mid`` -> ``out``).  ``x_parts``: 1 .. 3
    contiguous float32 CUDA tensors [B, C_i, H, W] read in place as their channel concatenation; ``h``, ``z``, ``rh``, ``mid``, ``out``:
    [B, h_channels, H, W], five different buffers; ``packed``: a mapping with PACKED_KEYS, flat float32 tensors in the layout of
    include/ftk.h.  No synchronisation, no allocation: capturable.  Every argument is checked before the device is touched."""
    from . import device as D

    ks = int(kernel_size)
    if ks not in N.FTK_SEP_CONV_GRU_KERNEL_SIZES:
        raise ValueError(f"kernel_size {kernel_size} is not supported: 3 and 5 are")
    x_parts = N.part_list(x_parts, "x", N.FTK_SEP_CONV_GRU_MAX_PARTS)
    dev = D._call_device(ctx, h)
    D._check("h", h, D._F32, (None, None, None, None), dev)
    B, Ch, H, W = (int(e) for e in h.shape)
    if min(B, Ch, H, W) < 1:
        raise ValueError(f"h must be a non-empty [B, h_channels, H, W] tensor (got {list(h.shape)})")
    if Ch > N.FTK_SEP_CONV_GRU_MAX_H_CHANNELS:
        raise ValueError(f"h_channels {Ch} above FTK_SEP_CONV_GRU_MAX_H_CHANNELS = {N.FTK_SEP_CONV_GRU_MAX_H_CHANNELS}")
    Cin = N.checked_channels("x", x_parts, B, H, W, dev) + Ch
    if Cin > N.FTK_SEP_CONV_GRU_MAX_IN_CHANNELS:
        raise ValueError(f"x_channels + h_channels = {Cin} above FTK_SEP_CONV_GRU_MAX_IN_CHANNELS = {N.FTK_SEP_CONV_GRU_MAX_IN_CHANNELS}")
    for name, t in (("z", z), ("rh", rh), ("mid", mid), ("out", out)):
        D._check(name, t, D._F32, (B, Ch, H, W), dev)
    for key in PACKED_KEYS:
        if key not in packed:
            raise ValueError(f"packed lacks {key!r}")
        rows = Ch if key.startswith("q") else 2 * Ch
        want = rows if "bias" in key else N.sep_conv_gru_packed_elements(rows, Cin, ks)
        D._check(f"packed[{key!r}]", packed[key], D._F32, (want,), dev)
    s = stream_or_current(h, stream)
    parts = N.part_array(x_parts)
    ptr = {key: C.c_void_p(packed[key].data_ptr()) for key in PACKED_KEYS}
    h_p, z_p, rh_p, mid_p, out_p = (C.c_void_p(t.data_ptr()) for t in (h, z, rh, mid, out))
    lib, sh = N.lib(), C.c_void_p(s.cuda_stream)
    for vertical, d, src, dst in ((0, "horizontal", h_p, mid_p), (1, "vertical", mid_p, out_p)):
        rc = lib.ftk_sep_conv_gru_gates_device(ctx.handle, sh, parts, len(x_parts), src, ptr["zr_" + d], ptr["zr_bias_" + d], Ch, ks, vertical, B, H, W,
                                               z_p, rh_p)
        N.check(rc, ctx.handle)
        rc = lib.ftk_sep_conv_gru_blend_device(ctx.handle, sh, parts, len(x_parts), rh_p, z_p, src, ptr["q_" + d], ptr["q_bias_" + d], Ch, ks, vertical,
                                               B, H, W, dst)
        N.check(rc, ctx.handle)
