"""``device.conv2d_device``: the torch device entry of the stock layers of RAFT's UpdateBlock (ftk_conv2d_device), and
``device.conv2d_strided_device``, the same layer with a stride, a residual and the image normalisation for RAFT's encoders
(ftk_conv2d_strided_device; its walk and refusals are tests/test_raft_encoder_cpu.py), ``device.conv2d_pool_device``, the
layer with a 2 x 2 max-pool in its epilogue, and ``device.channel_normalise_device``, both for SuperPoint (ftk_conv2d_pool_device and
ftk_channel_normalise_device; their walk and refusals are tests/test_superpoint_cpu.py).

It is re-exported by device.py and held to that module's rule: no ``data_ptr()`` of a tensor that did not pass ``device._check``.
It lives in a file of its own for the reason _device_sep_conv_gru.py gives; this entry's walk (the same recording stand-ins) and its
refusals are tests/test_update_block_cpu.py.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _native as N
from ._torch_call import stream_or_current


def _conv2d(ctx, parts, packed_weights, bias, kernel_size, relu, out_scale, out, stream, *, strided: bool, stride=1, residual=None, normalise=False,
            pool: bool = False) -> None:
    """The checks and the marshalling of the three conv entries; ``strided`` and ``pool`` say which of them calls, and so which ABI entry is
    called."""
    from . import device as D

    ks, st = int(kernel_size), int(stride)
    if ks not in N.FTK_CONV2D_KERNEL_SIZES:
        raise ValueError(f"kernel_size {kernel_size} is not supported: 1, 3 and 7 are")
    if strided and (st not in N.FTK_CONV2D_STRIDES or ks not in N.FTK_CONV2D_STRIDES[st]):
        raise ValueError(f"stride {stride} with kernel_size {ks} is not supported: stride 1, and stride 2 with kernel sizes 1 and 3, are")
    if pool and ks not in N.FTK_CONV2D_POOL_KERNEL_SIZES:
        raise ValueError(f"kernel_size {ks} is not supported with the max-pool: 1 and 3 are")
    if not math.isfinite(float(out_scale)):
        raise ValueError(f"out_scale must be finite (got {out_scale})")
    parts = N.part_list(parts, "the input", N.FTK_CONV2D_MAX_PARTS)
    dev = D._call_device(ctx, out)
    D._check("out", out, D._F32, (None, None, None, None), dev)
    B, Cout, OH, OW = (int(e) for e in out.shape)
    if min(B, Cout, OH, OW) < 1:
        raise ValueError(f"out must be a non-empty [B, out_channels, H, W] tensor (got {list(out.shape)})")
    if Cout > N.FTK_CONV2D_MAX_OUT_CHANNELS:
        raise ValueError(f"out_channels {Cout} above FTK_CONV2D_MAX_OUT_CHANNELS = {N.FTK_CONV2D_MAX_OUT_CHANNELS}")
    H, W = OH, OW
    if strided or pool:  # the input's sizes are parts[0]'s
        D._check("parts[0]", parts[0], D._F32, (B, None, None, None), dev)
        H, W = int(parts[0].shape[2]), int(parts[0].shape[3])
        if pool and (H // 2, W // 2) != (OH, OW):
            raise ValueError(f"out must be [B, out_channels, {H // 2}, {W // 2}] for parts[0] {list(parts[0].shape)} under a 2 x 2 max-pool (got "
                             f"{list(out.shape)})")
        if not pool and (-(-H // st), -(-W // st)) != (OH, OW):
            raise ValueError(f"out must be [B, out_channels, {-(-H // st)}, {-(-W // st)}] for parts[0] {list(parts[0].shape)} at stride {st} (got "
                             f"{list(out.shape)})")
    Cin = N.checked_channels("parts", parts, B, H, W, dev)
    if Cin > N.FTK_CONV2D_MAX_IN_CHANNELS:
        raise ValueError(f"in_channels {Cin} above FTK_CONV2D_MAX_IN_CHANNELS = {N.FTK_CONV2D_MAX_IN_CHANNELS}")
    D._check("packed_weights", packed_weights, D._F32, (N.conv2d_packed_elements(Cout, Cin, ks),), dev)
    D._check("bias", bias, D._F32, (Cout,), dev)
    if residual is not None:
        D._check("residual", residual, D._F32, (B, Cout, OH, OW), dev)
    s = stream_or_current(out, stream)
    layer = (ctx.handle, C.c_void_p(s.cuda_stream), N.part_array(parts), len(parts), C.c_void_p(packed_weights.data_ptr()), C.c_void_p(bias.data_ptr()), Cout, ks)
    sizes = (B, H, W, C.c_void_p(out.data_ptr()))
    if pool:
        rc = N.lib().ftk_conv2d_pool_device(*layer, 1 if relu else 0, *sizes)
    elif strided:
        rc = N.lib().ftk_conv2d_strided_device(*layer, st, 1 if relu else 0, float(out_scale), None if residual is None else C.c_void_p(residual.data_ptr()),
                                               1 if normalise else 0, *sizes)
    else:
        rc = N.lib().ftk_conv2d_device(*layer, 1 if relu else 0, float(out_scale), *sizes)
    N.check(rc, ctx.handle)


def conv2d_device(ctx, parts, packed_weights, bias, kernel_size: int, relu: bool, out_scale: float, out, stream=None) -> None:
    """One layer of update_block.py (a Conv2d of kernel size 1, 3 or 7, stride 1, zero padding ``kernel_size // 2``; with ``relu`` the
    ReLU after it; then ``out_scale *``, 1.0 everywhere but the mask head's last layer) in one launch on ``stream`` (a torch.cuda.Stream;
    default: torch's current stream).  ``parts``: 1 .. 3 contiguous float32 CUDA tensors [B, C_i, H, W] read in place as their channel
    concatenation; ``out``: [B, out_channels, H, W]; ``bias``: [out_channels]; ``packed_weights``: the flat float32 tensor in the layout
    of include/ftk.h.  No synchronisation, no allocation: capturable.  Every argument is checked before the device is touched."""
    _conv2d(ctx, parts, packed_weights, bias, kernel_size, relu, out_scale, out, stream, strided=False)


def conv2d_strided_device(ctx, parts, packed_weights, bias, kernel_size: int, stride: int, relu: bool, out_scale: float, residual, normalise: bool, out,
                          stream=None) -> None:
    """One layer of encoder.py: ``conv2d_device`` with a ``stride`` of 1 or 2 (2: kernel sizes 1 and 3), with ``residual`` (None or a
    contiguous float32 CUDA tensor of ``out``'s shape) added before the ReLU, and with ``normalise`` model.py:70-71's ``2 * (x / 255) - 1``
    applied to the in-image input values.  ``parts``: [B, C_i, H, W]; ``out``: [B, out_channels, ceil(H / stride), ceil(W / stride)].  The
    weights are BatchNorm-folded by the caller and packed as for ``conv2d_device``.  One launch, no synchronisation, no allocation:
    capturable.  Every argument is checked before the device is touched."""
    _conv2d(ctx, parts, packed_weights, bias, kernel_size, relu, out_scale, out, stream, strided=True, stride=stride, residual=residual, normalise=normalise)


def conv2d_pool_device(ctx, parts, packed_weights, bias, kernel_size: int, relu: bool, out, stream=None) -> None:
    """One layer of SuperPoint's VGG with the pool after it: ``conv2d_device`` (kernel size 1 or 3; there is no ``out_scale``) followed by
    ``max_pool2d(2, 2)``, in one launch that never stores the tensor before the pool.  ``parts``: [B, C_i, H, W] with H, W >= 2; ``out``:
    [B, out_channels, H // 2, W // 2]: a last odd row or column is dropped.  A NaN propagates and the first of equal maxima wins, as in
    torch.  No synchronisation, no allocation: capturable.  Every argument is checked before the device is touched."""
    _conv2d(ctx, parts, packed_weights, bias, kernel_size, relu, 1.0, out, stream, strided=False, pool=True)


def channel_normalise_device(ctx, x, out, stream=None) -> None:
    """The L2 normalisation of a dense descriptor map over its channels (``torch.nn.functional.normalize(dim=1)`` with the summation order
    of DESIGN.md 5.25), written channel-last: ``x`` contiguous float32 CUDA [D, Hc, Wc], ``out`` [Hc, Wc, D]; ``out.permute(2, 0, 1)`` is
    the view ``KeypointDecoder.decode`` reads with coalesced loads.  One launch on ``stream`` (default: torch's current stream), no
    synchronisation, no allocation: capturable.  Every argument is checked before the device is touched."""
    from . import device as D

    dev = D._call_device(ctx, x)
    D._check("x", x, D._F32, (None, None, None), dev)
    d, hc, wc = (int(e) for e in x.shape)
    if not 1 <= d <= N.FTK_KEYPOINT_DECODE_MAX_CHANNELS:
        raise ValueError(f"x must have 1 .. FTK_KEYPOINT_DECODE_MAX_CHANNELS = {N.FTK_KEYPOINT_DECODE_MAX_CHANNELS} channels (got {d})")
    if min(hc, wc) < 1:
        raise ValueError(f"x must be a non-empty [D, Hc, Wc] tensor (got {list(x.shape)})")
    D._check("out", out, D._F32, (hc, wc, d), dev)
    s = stream_or_current(x, stream)
    N.check(N.lib().ftk_channel_normalise_device(ctx.handle, C.c_void_p(s.cuda_stream), C.c_void_p(x.data_ptr()), d, hc, wc, C.c_void_p(out.data_ptr())),
            ctx.handle)
