"""``device.lightglue_confidence_device``, ``device.lightglue_adapt_step_device``, ``device.transformer_layer_adaptive_device`` and
``device.lightglue_finish_device``: the torch device entries of LightGlue's adaptive depth and width.

They are re-exported by device.py and held to that module's rule: no ``data_ptr()`` of a tensor that did not pass ``device._check``.  They
live in a file of their own for _device_klt_video.py's reason; their walk and their refusals are tests/test_lightglue_adaptive_args_cpu.py.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _native as N
from ._device_transformer import check_heads, check_rows
from ._torch_call import pointer, stream_or_current


def stop_threshold(layer: int, n_layers: int) -> float:
    """Upstream's ``confidence_threshold``: ``clip(0.8 + 0.1 exp(-4 i / L), 0, 1)`` in float64, as the float32 the library receives."""
    import numpy as np

    return float(np.float32(min(max(0.8 + 0.1 * math.exp(-4.0 * layer / n_layers), 0.0), 1.0)))


def check_confidence(name: str, value) -> float:
    """``depth_confidence`` / ``width_confidence``: a number at most 1; <= 0 switches the mechanism off."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or math.isnan(value) or value > 1:
        raise ValueError(f"{name} must be a number <= 1 (<= 0: off) (got {value!r})")
    return float(value)


def check_layer_index(name: str, value, least: int) -> int:
    if isinstance(value, bool) or not isinstance(value, int) or not least <= value <= N.FTK_LIGHTGLUE_MAX_LAYERS - 1 + least:
        raise ValueError(f"{name} must be an integer in {least} .. {N.FTK_LIGHTGLUE_MAX_LAYERS - 1 + least} (got {value!r})")
    return value


def check_min_keypoints(value) -> int:
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value < 2 ** 31:
        raise ValueError(f"pruning_min_keypoints must be an integer >= 0 (got {value!r})")
    return value


def _workspace(D, workspace, m, n, d, heads, dev):
    D._check("workspace", workspace, D._KEYS, (None,), dev, min_numel=-(-N.lightglue_adaptive_workspace_bytes(m, n, d, heads) // 8))


def _sets(D, ctx, desc0, desc1, heads, names=("desc0", "desc1")):
    """The checks every entry shares: (device index, M, N, D, dh)."""
    dev = D._call_device(ctx, desc0)
    D._check(names[0], desc0, D._F32, (None, None), dev)
    m, d = int(desc0.shape[0]), int(desc0.shape[1])
    D._check(names[1], desc1, D._F32, (None, d), dev)
    n = int(desc1.shape[0])
    check_rows("desc0 and desc1", m, n)
    dh = None if heads is None else check_heads(d, heads)
    if heads is None and not 1 <= d <= N.FTK_TRANSFORMER_MAX_DIM:
        raise ValueError(f"the descriptors must have 1 .. FTK_TRANSFORMER_MAX_DIM = {N.FTK_TRANSFORMER_MAX_DIM} columns (got {d})")
    return dev, m, n, d, dh


def lightglue_confidence_args(ctx, desc0, desc1, token_w, token_b, match_w, match_b, live0, live1, gate, conf, mt, stream=None):
    """Checks one ftk_lightglue_confidence_device call and returns its marshalled arguments."""
    from . import device as D

    dev, m, n, d, _ = _sets(D, ctx, desc0, desc1, None)
    D._check("token_w", token_w, D._F32, (d,), dev)
    D._check("token_b", token_b, D._F32, (1,), dev)
    D._check("match_w", match_w, D._F32, (d,), dev)
    D._check("match_b", match_b, D._F32, (1,), dev)
    for name, word in (("live0", live0), ("live1", live1), ("gate", gate)):
        if word is not None:
            D._check(name, word, D._I32, (1,), dev)
    D._check("conf", conf, D._F32, (m + n,), dev)
    D._check("mt", mt, D._F32, (m + n,), dev)
    st = stream_or_current(desc0, stream)
    return (ctx.handle, C.c_void_p(st.cuda_stream), pointer(desc0), m, pointer(desc1), n, d, pointer(token_w), pointer(token_b), pointer(match_w),
            pointer(match_b), pointer(live0), pointer(live1), pointer(gate), pointer(conf), pointer(mt))


def lightglue_confidence_device(ctx, desc0, desc1, token_w, token_b, match_w, match_b, live0, live1, gate, conf, mt, stream=None) -> None:
    """ftk_lightglue_confidence_device: ``conf`` and ``mt`` (float32 [M + N], the second set from M) of the live rows of ``desc0`` [M, D]
    and ``desc1`` [N, D]: ``sigmoid_c`` of the fmaf chains over the columns from ``token_b`` / ``match_b`` [1] with ``token_w`` /
    ``match_w`` [D].  ``live0`` / ``live1`` / ``gate``: int32 [1] device tensors or None (all rows; never gated).  1 launch on
    ``stream``; every argument is checked before the device is touched."""
    args = lightglue_confidence_args(ctx, desc0, desc1, token_w, token_b, match_w, match_b, live0, live1, gate, conf, mt, stream)
    N.check(N.lib().ftk_lightglue_confidence_device(*args), ctx.handle)


def transformer_layer_adaptive_args(ctx, desc0, desc1, heads, enc0, enc1, weights, live0, live1, gate, workspace, stream=None):
    """Checks one ftk_transformer_layer_adaptive_device call and returns its marshalled arguments."""
    from . import device as D

    dev, m, n, d, dh = _sets(D, ctx, desc0, desc1, heads)
    D._check("enc0", enc0, D._F32, (2, m, dh), dev)
    D._check("enc1", enc1, D._F32, (2, n, dh), dev)
    D._check("weights", weights, D._F32, (N.transformer_layer_weight_offsets(d)[2],), dev)
    for name, word in (("live0", live0), ("live1", live1), ("gate", gate)):
        D._check(name, word, D._I32, (1,), dev)
    D._check("workspace", workspace, D._KEYS, (None,), dev, min_numel=-(-N.transformer_layer_workspace_bytes(m, n, d, heads) // 8))
    st = stream_or_current(desc0, stream)
    return (ctx.handle, C.c_void_p(st.cuda_stream), pointer(desc0), m, pointer(desc1), n, d, heads, pointer(enc0), pointer(enc1), pointer(weights),
            pointer(live0), pointer(live1), pointer(gate), pointer(workspace))


def transformer_layer_adaptive_device(ctx, desc0, desc1, heads, enc0, enc1, weights, live0, live1, gate, workspace, stream=None) -> None:
    """ftk_transformer_layer_adaptive_device: ``transformer_layer_device`` in place on ``desc0`` and ``desc1``, with the live counts
    ``live0`` / ``live1`` (int32 [1], required) as the counts; nothing is done when ``gate`` (int32 [1]) is not 0, and no workgroup
    works on rows that all lie at or behind their live count.  12 launches; capturable."""
    args = transformer_layer_adaptive_args(ctx, desc0, desc1, heads, enc0, enc1, weights, live0, live1, gate, workspace, stream)
    N.check(N.lib().ftk_transformer_layer_adaptive_device(*args), ctx.handle)


def lightglue_adapt_step_args(ctx, heads, layer, conf, mt, count0, count1, state, threshold, depth_confidence, width_confidence, min_keypoints, src,
                              dst, layers0, layers1, workspace, stream=None):
    """Checks one ftk_lightglue_adapt_step_device call and returns its marshalled arguments.  ``src`` and ``dst``: the two halves of the
    pair, each ``(desc0, desc1, enc0, enc1, ind0, ind1)``."""
    from . import device as D

    if len(src) != 6 or len(dst) != 6:
        raise ValueError("src and dst must each be (desc0, desc1, enc0, enc1, ind0, ind1)")
    dev, m, n, d, dh = _sets(D, ctx, src[0], src[1], heads, ("src desc0", "src desc1"))
    check_layer_index("layer", layer, 0)
    depth, width = check_confidence("depth_confidence", depth_confidence), check_confidence("width_confidence", width_confidence)
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 <= threshold <= 1.0:
        raise ValueError(f"threshold must be a number in 0 .. 1 (got {threshold!r})")
    check_min_keypoints(min_keypoints)
    for which, half in (("src", src), ("dst", dst)):
        D._check(f"{which} desc0", half[0], D._F32, (m, d), dev)
        D._check(f"{which} desc1", half[1], D._F32, (n, d), dev)
        D._check(f"{which} enc0", half[2], D._F32, (2, m, dh), dev)
        D._check(f"{which} enc1", half[3], D._F32, (2, n, dh), dev)
        D._check(f"{which} ind0", half[4], D._I32, (m,), dev)
        D._check(f"{which} ind1", half[5], D._I32, (n,), dev)
    for k, (a, b) in enumerate(zip(src, dst)):
        if a is b:
            raise ValueError(f"src[{k}] and dst[{k}] are one buffer: the gather is not in place")
    D._check("conf", conf, D._F32, (m + n,), dev)
    D._check("mt", mt, D._F32, (m + n,), dev)
    for name, word in (("count0", count0), ("count1", count1)):
        if word is not None:
            D._check(name, word, D._I32, (1,), dev)
    D._check("state", state, D._I32, (N.FTK_LIGHTGLUE_STATE_WORDS,), dev)
    D._check("layers0", layers0, D._I32, (m,), dev)
    D._check("layers1", layers1, D._I32, (n,), dev)
    _workspace(D, workspace, m, n, d, heads, dev)
    st = stream_or_current(src[0], stream)
    return ((ctx.handle, C.c_void_p(st.cuda_stream), m, n, d, heads, layer, pointer(conf), pointer(mt), pointer(count0), pointer(count1), pointer(state),
             C.c_float(threshold), C.c_float(depth), C.c_float(width), min_keypoints) + tuple(pointer(t) for t in src) + tuple(pointer(t) for t in dst)
            + (pointer(layers0), pointer(layers1), pointer(workspace)))


def lightglue_adapt_step_device(ctx, heads, layer, conf, mt, count0, count1, state, threshold, depth_confidence, width_confidence, min_keypoints, src, dst,
                                layers0, layers1, workspace, stream=None) -> None:
    """ftk_lightglue_adapt_step_device: layer ``layer``'s stop test and pruning on ``conf`` and ``mt``,
    then the stable gather of the kept rows of ``src`` to the front of ``dst``.  ``state``: int32 [4] (live0, live1, stopped,
    stop_layer).  2 launches; capturable."""
    args = lightglue_adapt_step_args(ctx, heads, layer, conf, mt, count0, count1, state, threshold, depth_confidence, width_confidence, min_keypoints,
                                     src, dst, layers0, layers1, workspace, stream)
    N.check(N.lib().ftk_lightglue_adapt_step_device(*args), ctx.handle)


def lightglue_finish_args(ctx, desc0, desc1, heads, head_w, head_b, state, ind0, ind1, min_score, workspace, scores, match_index, status, layers0,
                          layers1, stream=None):
    """Checks one ftk_lightglue_finish_device call and returns its marshalled arguments."""
    from . import device as D

    dev, m, n, d, _ = _sets(D, ctx, desc0, desc1, heads)
    D._check("head_w", head_w, D._F32, (None, d + 1, d), dev)
    n_layers = int(head_w.shape[0])
    check_layer_index("the number of layers", n_layers, 1)
    D._check("head_b", head_b, D._F32, (n_layers, d + 1), dev)
    D._check("state", state, D._I32, (N.FTK_LIGHTGLUE_STATE_WORDS,), dev)
    D._check("ind0", ind0, D._I32, (m,), dev)
    D._check("ind1", ind1, D._I32, (n,), dev)
    if isinstance(min_score, bool) or not isinstance(min_score, (int, float)) or math.isnan(min_score):
        raise ValueError(f"min_score must be a number (got {min_score!r})")
    _workspace(D, workspace, m, n, d, heads, dev)
    D._check("scores", scores, D._F32, (m + 1, n + 1), dev)
    D._check("match_index", match_index, D._I32, (m,), dev)
    D._check("status", status, D._U8, (m,), dev)
    D._check("layers0", layers0, D._I32, (m,), dev)
    D._check("layers1", layers1, D._I32, (n,), dev)
    st = stream_or_current(desc0, stream)
    return (ctx.handle, C.c_void_p(st.cuda_stream), pointer(desc0), m, pointer(desc1), n, d, heads, n_layers, pointer(head_w), pointer(head_b),
            pointer(state), pointer(ind0), pointer(ind1), C.c_float(min_score), pointer(workspace), pointer(scores), pointer(match_index),
            pointer(status), pointer(layers0), pointer(layers1))


def lightglue_finish_device(ctx, desc0, desc1, heads, head_w, head_b, state, ind0, ind1, min_score, workspace, scores, match_index, status, layers0,
                            layers1, stream=None) -> None:
    """ftk_lightglue_finish_device: the head of the stop layer out of ``head_w`` [L, D + 1, D] and ``head_b`` [L, D + 1], the assignment
    head and the matcher on the compacted sets, and the map back: ``scores`` [M + 1, N + 1] in compacted layout, ``match_index`` int32 [M]
    and ``status`` uint8 [M] in original indices, ``layers0`` / ``layers1`` of the rows that stayed.  Capturable once the context's
    matcher workspace holds the size."""
    args = lightglue_finish_args(ctx, desc0, desc1, heads, head_w, head_b, state, ind0, ind1, min_score, workspace, scores, match_index, status, layers0,
                                 layers1, stream)
    N.check(N.lib().ftk_lightglue_finish_device(*args), ctx.handle)
