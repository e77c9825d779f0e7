"""``device.keypoint_decode_device``: the torch device entry of the keypoint decoder (ftk_keypoint_decode_device).

It is re-exported by device.py and held to that module's rule: no ``data_ptr()`` of a tensor that did not pass ``device._check``.  It lives
in a file of its own for _device_klt_video.py's reason; its walk and its refusals are tests/test_keypoint_decode_args_cpu.py.
"""
from __future__ import annotations

import ctypes as C
import math

from . import _native as N
from ._torch_call import pointer, stream_or_current

LAYOUTS = ("chw", "hwc")
MAX_CELLS = 65536 // N.FTK_KEYPOINT_DECODE_CELL


def check_options(max_keypoints, min_score, min_distance, border):
    """(max_keypoints, min_score, min_distance, border) as the ABI takes them, or the ValueError."""
    for name, v in (("max_keypoints", max_keypoints), ("min_distance", min_distance), ("border", border)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an integer (got {v!r})")
    if not 1 <= max_keypoints <= N.FTK_KEYPOINT_DECODE_MAX_KEYPOINTS:
        raise ValueError(f"max_keypoints must be in 1 .. FTK_KEYPOINT_DECODE_MAX_KEYPOINTS = {N.FTK_KEYPOINT_DECODE_MAX_KEYPOINTS} (got {max_keypoints})")
    try:
        s = float(min_score)
    except (TypeError, ValueError):
        s = math.nan
    if not math.isfinite(s) or abs(s) > 3.0e38:
        raise ValueError(f"min_score must be a finite number (got {min_score!r})")
    if border < 0:
        raise ValueError(f"border must not be negative (got {border})")
    if not -(1 << 31) <= min_distance < (1 << 31) or border >= (1 << 31):
        raise ValueError(f"min_distance and border must fit an int32 (got {min_distance}, {border})")
    return max_keypoints, s, min_distance, border


def check_grid(cell_rows: int, cell_cols: int, min_distance: int) -> None:
    """The limits of the cell grid: H, W <= 65 536 and the survivor bound of the 8 cell_rows x 8 cell_cols image."""
    if not (1 <= cell_rows <= MAX_CELLS and 1 <= cell_cols <= MAX_CELLS):
        raise ValueError(f"semi must cover 1 .. {MAX_CELLS} cells along either axis: the image is at most 65536 x 65536 (got {cell_rows} x {cell_cols} cells)")
    rows, cols, d = 8 * cell_rows, 8 * cell_cols, max(int(min_distance), 1)
    bound = -(-rows // d) * -(-cols // d)
    if bound > N.FTK_HARRIS_DEVICE_MAX_SURVIVORS:
        raise ValueError(f"a {rows} x {cols} image at min_distance {int(min_distance)} can hold {bound} keypoints, above "
                         f"FTK_HARRIS_DEVICE_MAX_SURVIVORS = {N.FTK_HARRIS_DEVICE_MAX_SURVIVORS}: raise min_distance")


def keypoint_decode_args(ctx, semi, desc, max_keypoints: int, min_score: float, min_distance: int, border: int, workspace, uv, scores, descriptors, count,
                         heatmap=None, occupied=None, occupied_mask=None, desc_layout: str = "chw", stream=None):
    """Checks one ftk_keypoint_decode_device call and returns its marshalled arguments."""
    from . import device as D

    k, s, distance, border = check_options(max_keypoints, min_score, min_distance, border)
    if desc_layout not in LAYOUTS:
        raise ValueError(f"desc_layout must be one of {list(LAYOUTS)} (got {desc_layout!r})")
    if occupied is None and occupied_mask is not None:
        raise ValueError("occupied_mask without occupied: the mask selects among the occupied points")
    dev = D._call_device(ctx, semi)
    D._check("semi", semi, D._F32, (65, None, None), dev)
    hc, wc = int(semi.shape[1]), int(semi.shape[2])
    check_grid(hc, wc, distance)
    D._check("desc", desc, D._F32, (None, hc, wc) if desc_layout == "chw" else (hc, wc, None), dev)
    d = int(desc.shape[0 if desc_layout == "chw" else 2])
    if not 1 <= d <= N.FTK_KEYPOINT_DECODE_MAX_CHANNELS:
        raise ValueError(f"desc must have 1 .. FTK_KEYPOINT_DECODE_MAX_CHANNELS = {N.FTK_KEYPOINT_DECODE_MAX_CHANNELS} channels (got {d})")
    strides = (hc * wc, wc, 1) if desc_layout == "chw" else (1, wc * d, d)
    n = 0
    if occupied is not None:
        D._check("occupied", occupied, D._F32, (None, 2), dev)
        n = int(occupied.shape[0])
        if occupied_mask is not None:
            D._check("occupied_mask", occupied_mask, D._U8, (n,), dev)
    D._check("workspace", workspace, D._KEYS, (None,), dev, min_numel=-(-N.keypoint_decode_workspace_bytes(hc, wc, distance, n) // 8))
    D._check("uv", uv, D._F32, (k, 2), dev)
    D._check("scores", scores, D._F32, (k,), dev)
    D._check("descriptors", descriptors, D._F32, (k, d), dev)
    D._check("count", count, D._I32, (1,), dev)
    if heatmap is not None:
        D._check("heatmap", heatmap, D._F32, (8 * hc, 8 * wc), dev)
    st = stream_or_current(semi, stream)
    p = pointer
    return (ctx.handle, C.c_void_p(st.cuda_stream), p(semi), hc, wc, p(desc), d, strides[0], strides[1], strides[2], k, C.c_float(s), distance, border,
            p(occupied), p(occupied_mask) if n > 0 else None, n, p(workspace), p(uv), p(scores), p(descriptors), p(count), p(heatmap))


def keypoint_decode_device(ctx, semi, desc, max_keypoints: int, min_score: float, min_distance: int, border: int, workspace, uv, scores, descriptors, count,
                           heatmap=None, occupied=None, occupied_mask=None, desc_layout: str = "chw", stream=None) -> None:
    """ftk_keypoint_decode_device: the detector head's logits ``semi`` (contiguous float32 CUDA [65, Hc, Wc], channel 64 the dustbin) and the
    coarse descriptor map ``desc`` (contiguous float32, [D, Hc, Wc] with ``desc_layout`` "chw" or [Hc, Wc, D] with "hwc"; the same bits
    either way) to ``uv`` float32 [max_keypoints, 2] ((col, row) of the strongest keypoints of the 8 Hc x 8 Wc image, strongest first),
    ``scores`` float32 [max_keypoints], ``descriptors`` float32 [max_keypoints, D] (bilinear samples, L2-normalised) and ``count`` int32
    [1]; the rows behind ``count`` are zeros.  ``heatmap``: float32 [8 Hc, 8 Wc] for every pixel's score, or None.  ``occupied`` /
    ``occupied_mask``: as ``harris_detect_device`` takes them.  ``workspace``: int64 or uint64 CUDA tensor of at least
    ``_native.keypoint_decode_workspace_bytes(Hc, Wc, min_distance, n_occupied) / 8`` elements.  7 launches (10 with occupied points) on
    ``stream`` (default: torch's current stream), no synchronisation, no allocation: capturable.  Every argument is checked before the
    device is touched."""
    args = keypoint_decode_args(ctx, semi, desc, max_keypoints, min_score, min_distance, border, workspace, uv, scores, descriptors, count, heatmap,
                                occupied, occupied_mask, desc_layout, stream)
    N.check(N.lib().ftk_keypoint_decode_device(*args), ctx.handle)
