"""``device.attention_device``, ``device.linear_device`` and ``device.transformer_layer_device``: the torch device entries of LightGlue's
transformer layer (ftk_attention_device, ftk_linear_device, ftk_transformer_layer_device).

They are re-exported by device.py and held to that module's rule: no ``data_ptr()`` of a tensor that did not pass ``device._check``.  They
live in a file of their own for _device_klt_video.py's reason; their walk and their refusals are tests/test_transformer_args_cpu.py.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _native as N
from ._torch_call import pointer, stream_or_current


def check_scale(name: str, scale) -> float:
    """A scale as the ABI takes it, or the ValueError."""
    try:
        s = float(scale)
    except (TypeError, ValueError):
        s = math.nan
    if isinstance(scale, bool) or not math.isfinite(s) or not 0.0 < s <= 3.0e38:
        raise ValueError(f"{name} must be a finite number > 0 (got {scale!r})")
    return s


def check_rows(what: str, *rows: int) -> None:
    if not all(1 <= r <= N.FTK_TRANSFORMER_MAX_ROWS for r in rows):
        raise ValueError(f"{what} must have 1 .. FTK_TRANSFORMER_MAX_ROWS = {N.FTK_TRANSFORMER_MAX_ROWS} rows (got {' and '.join(str(r) for r in rows)})")


def check_heads(dim: int, heads) -> int:
    """The limits of include/ftk.h on (D, h); the head dimension."""
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
        raise ValueError(f"num_heads must be a positive integer (got {heads!r})")
    if not 1 <= dim <= N.FTK_TRANSFORMER_MAX_DIM:
        raise ValueError(f"the descriptors must have 1 .. FTK_TRANSFORMER_MAX_DIM = {N.FTK_TRANSFORMER_MAX_DIM} columns (got {dim})")
    if dim % heads != 0:
        raise ValueError(f"num_heads = {heads} must divide D = {dim}")
    dh = dim // heads
    if dh % 2 != 0 or not 2 <= dh <= N.FTK_TRANSFORMER_MAX_HEAD_DIM:
        raise ValueError(f"the head dimension must be even and in 2 .. FTK_TRANSFORMER_MAX_HEAD_DIM = {N.FTK_TRANSFORMER_MAX_HEAD_DIM} (got {dh})")
    return dh


def attention_args(ctx, q, k, v, count, pre_scale, post_scale, out, stream=None):
    """Checks one ftk_attention_device call and returns its marshalled arguments."""
    from . import device as D

    pre = check_scale("pre_scale", pre_scale)
    dev = D._call_device(ctx, q)
    D._check("q", q, D._F32, (None, None, None), dev)
    m, h, dh = (int(e) for e in q.shape)
    D._check("k", k, D._F32, (None, h, dh), dev)
    n = int(k.shape[0])
    D._check("v", v, D._F32, (n, h, dh), dev)
    check_rows("q and k", m, n)
    if h < 1 or dh < 1:
        raise ValueError(f"q must have at least one head and one channel (got {[m, h, dh]})")
    check_heads(h * dh, h)
    post = check_scale("post_scale", dh ** -0.5 if post_scale is None else post_scale)
    if count is not None:
        D._check("count", count, D._I32, (1,), dev)
    D._check("out", out, D._F32, (m, h, dh), dev)
    st = stream_or_current(q, stream)
    return (ctx.handle, C.c_void_p(st.cuda_stream), pointer(q), m, pointer(k), pointer(v), n, h, dh, pointer(count), C.c_float(pre), C.c_float(post),
            pointer(out))


def attention_device(ctx, q, k, v, count, pre_scale, post_scale, out, stream=None) -> None:
    """ftk_attention_device: ``out`` [M, h, dh] = softmax over the first ``clamp(count, 0, N)`` keys of ``(q pre)(k pre)^T post``, times
    ``v``, per head.  ``q`` [M, h, dh], ``k`` and ``v`` [N, h, dh]: contiguous float32 CUDA tensors; ``count``: an int32 [1] device tensor
    or None; ``post_scale`` None: ``dh ** -0.5``.  1 launch on ``stream`` (default: torch's current stream), no synchronisation, no
    allocation: capturable.  Every argument is checked before the device is touched."""
    args = attention_args(ctx, q, k, v, count, pre_scale, post_scale, out, stream)
    N.check(N.lib().ftk_attention_device(*args), ctx.handle)


def linear_args(ctx, x, weight, bias, out, stream=None):
    """Checks one ftk_linear_device call and returns its marshalled arguments."""
    from . import device as D

    dev = D._call_device(ctx, x)
    D._check("x", x, D._F32, (None, None), dev)
    rows, k = int(x.shape[0]), int(x.shape[1])
    D._check("weight", weight, D._F32, (None, k), dev)
    outs = int(weight.shape[0])
    D._check("bias", bias, D._F32, (outs,), dev)
    check_rows("x", rows)
    if not (1 <= k <= N.FTK_TRANSFORMER_MAX_DIM and 1 <= outs <= N.FTK_TRANSFORMER_MAX_DIM):
        raise ValueError(f"weight must be [1 .. FTK_TRANSFORMER_MAX_DIM, 1 .. FTK_TRANSFORMER_MAX_DIM = {N.FTK_TRANSFORMER_MAX_DIM}] (got {[outs, k]})")
    D._check("out", out, D._F32, (rows, outs), dev)
    st = stream_or_current(x, stream)
    return (ctx.handle, C.c_void_p(st.cuda_stream), pointer(x), rows, k, pointer(weight), pointer(bias), outs, pointer(out))


def linear_device(ctx, x, weight, bias, out, stream=None) -> None:
    """ftk_linear_device: ``out`` [rows, O] = ``x`` [rows, K] ``weight``^T [O, K] + ``bias`` [O], each output the fmaf chain of DESIGN.md
    5.24 from its bias.  1 launch; every argument is checked before the device is touched."""
    args = linear_args(ctx, x, weight, bias, out, stream)
    N.check(N.lib().ftk_linear_device(*args), ctx.handle)


def transformer_layer_args(ctx, desc0, desc1, heads, enc0, enc1, weights, count0, count1, workspace, out0, out1, stream=None):
    """Checks one ftk_transformer_layer_device call and returns its marshalled arguments."""
    from . import device as D

    dev = D._call_device(ctx, desc0)
    D._check("desc0", desc0, D._F32, (None, None), dev)
    m, d = int(desc0.shape[0]), int(desc0.shape[1])
    D._check("desc1", desc1, D._F32, (None, d), dev)
    n = int(desc1.shape[0])
    check_rows("desc0 and desc1", m, n)
    dh = check_heads(d, heads)
    D._check("enc0", enc0, D._F32, (2, m, dh), dev)
    D._check("enc1", enc1, D._F32, (2, n, dh), dev)
    D._check("weights", weights, D._F32, (N.transformer_layer_weight_offsets(d)[2],), dev)
    if count0 is not None:
        D._check("count0", count0, D._I32, (1,), dev)
    if count1 is not None:
        D._check("count1", count1, D._I32, (1,), dev)
    D._check("workspace", workspace, D._KEYS, (None,), dev, min_numel=-(-N.transformer_layer_workspace_bytes(m, n, d, heads) // 8))
    D._check("out0", out0, D._F32, (m, d), dev)
    D._check("out1", out1, D._F32, (n, d), dev)
    st = stream_or_current(desc0, stream)
    return (ctx.handle, C.c_void_p(st.cuda_stream), pointer(desc0), m, pointer(desc1), n, d, heads, pointer(enc0), pointer(enc1), pointer(weights),
            pointer(count0), pointer(count1), pointer(workspace), pointer(out0), pointer(out1))


def transformer_layer_device(ctx, desc0, desc1, heads, enc0, enc1, weights, count0, count1, workspace, out0, out1, stream=None) -> None:
    """ftk_transformer_layer_device: one LightGlue layer on ``desc0`` (contiguous float32 CUDA [M, D]) and ``desc1`` ([N, D]) into ``out0``
    and ``out1`` of the same shapes.  ``enc0`` [2, M, dh], ``enc1`` [2, N, dh]: the rotary encoding's cos and sin.  ``weights``: the flat
    float32 tensor ``TransformerLayer.from_state_dict`` packs (``_native.transformer_layer_weight_offsets``).  ``count0`` / ``count1``:
    int32 [1] device tensors or None.  ``workspace``: int64 or uint64 CUDA tensor of at least
    ``_native.transformer_layer_workspace_bytes(M, N, D, heads) / 8`` elements.  12 launches on ``stream`` (default: torch's current
    stream), no synchronisation, no allocation: capturable.  Every argument is checked before the device is touched."""
    args = transformer_layer_args(ctx, desc0, desc1, heads, enc0, enc1, weights, count0, count1, workspace, out0, out1, stream)
    N.check(N.lib().ftk_transformer_layer_device(*args), ctx.handle)
