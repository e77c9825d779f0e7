"""``device.epipolar_ransac_device``: the torch device entry of two-view outlier rejection (ftk_epipolar_ransac_device).

It is re-exported by device.py and held to that module's rule: no ``datapointer()`` of a tensor that did not pass ``device._check``.
It lives in a file of its own because tests/test_device_args_cpu.py walks the entries DEFINED in device.py against a closed table;
this entry's walk (the same recording stand-ins) and its refusals are tests/test_epipolar_args_cpu.py.
"""
from __future__ import annotations

import ctypes as C

from . import _native as N
from ._torch_call import pointer, stream_or_current

SEED_ARG = 10  # where the seed sits in the marshalled arguments (KltVideoTracker replaces it per frame)


def check_sizes(image_size, threshold, hypotheses, seed):
    """(rows, cols, threshold, hypotheses, seed) as the ABI takes them, or the ValueError: before anything touches a device."""
    try:
        rows, cols = (int(e) for e in image_size)
    except (TypeError, ValueError):
        raise ValueError(f"image_size must be (H, W) (got {image_size!r})") from None
    if not (1 <= rows <= 65536 and 1 <= cols <= 65536):
        raise ValueError(f"image_size must be (H, W) with both in 1 .. 65536 (got {image_size!r})")
    t = float(threshold)
    if not 0.0 <= t <= 3.0e38:
        raise ValueError(f"threshold must be a finite number of pixels >= 0 (got {threshold})")
    k = int(hypotheses)
    if not 1 <= k <= N.FTK_EPIPOLAR_MAX_HYPOTHESES:
        raise ValueError(f"hypotheses must be in 1 .. FTK_EPIPOLAR_MAX_HYPOTHESES = {N.FTK_EPIPOLAR_MAX_HYPOTHESES} (got {hypotheses})")
    if not 0 <= int(seed) <= 0xFFFFFFFF:
        raise ValueError(f"seed must be a uint32 (got {seed})")
    return rows, cols, t, k, int(seed)


def ransac_inputs(ctx, ref_uv, cur_uv, status, sizes, stream):
    """What the checks of ftk_epipolar_ransac_device and ftk_two_view_ransac_device share after ``sizes = check_sizes(...)``: the three input
    tensors, the limit of n and the choice of stream.  Returns (device.py, the device the other tensors must be on, n, hypotheses, the
    marshalled arguments up to and including the seed); the caller checks its workspace and outputs against them and appends their pointers."""
    from . import device as D

    rows, cols, t, k, seed = sizes
    dev = D._call_device(ctx, ref_uv)
    D._check("ref_uv", ref_uv, D._F32, (None, 2), dev)
    n = int(ref_uv.shape[0])
    if not 1 <= n <= N.FTK_TRACK_TABLE_MAX_SLOTS:
        raise ValueError(f"ref_uv must have 1 .. FTK_TRACK_TABLE_MAX_SLOTS = {N.FTK_TRACK_TABLE_MAX_SLOTS} points (got {n})")
    D._check("cur_uv", cur_uv, D._F32, (n, 2), dev)
    D._check("status", status, D._U8, (n,), dev)
    s = stream_or_current(ref_uv, stream)
    head = (ctx.handle, C.c_void_p(s.cuda_stream), pointer(ref_uv), pointer(cur_uv), pointer(status), n, rows, cols, C.c_float(t), k, C.c_uint32(seed))
    return D, dev, n, k, head


def epipolar_ransac_args(ctx, ref_uv, cur_uv, status, image_size, threshold: float, hypotheses: int, seed: int, workspace, best, n_inliers, F,
                         counts=None, models=None, stream=None):
    """Checks one ftk_epipolar_ransac_device call and returns its marshalled arguments (KltVideoTracker keeps them: its tensors are fixed)."""
    D, dev, n, k, head = ransac_inputs(ctx, ref_uv, cur_uv, status, check_sizes(image_size, threshold, hypotheses, seed), stream)
    D._check("workspace", workspace, D._KEYS, (None,), dev, min_numel=-(-N.epipolar_workspace_bytes(n, k) // 8))
    D._check("best", best, D._I32, (1,), dev)
    D._check("n_inliers", n_inliers, D._I32, (1,), dev)
    D._check("F", F, D._F32, (3, 3), dev)
    if counts is not None:
        D._check("counts", counts, D._I32, (k,), dev)
    if models is not None:
        D._check("models", models, D._F32, (k, 9), dev)
    return head + (pointer(workspace), pointer(best), pointer(n_inliers), pointer(F), pointer(counts), pointer(models))


def epipolar_ransac_device(ctx, ref_uv, cur_uv, status, image_size, threshold: float, hypotheses: int, seed: int, workspace, best, n_inliers, F,
                           counts=None, models=None, stream=None) -> None:
    """ftk_epipolar_ransac_device: RANSAC on the fundamental matrix over the correspondences ``ref_uv[i] -> cur_uv[i]`` (contiguous float32
    CUDA [n, 2], (u, v) pixels) whose ``status`` (uint8 [n]) is TRACKED; ``status`` is rewritten in place (a participant that is no inlier
    of the winning hypothesis becomes LARGE_RESIDUAL), ``best`` / ``n_inliers`` (int32 [1]) and ``F`` (float32 [3, 3], pixel units,
    x_cur^T F x_ref = 0) receive the winner, ``counts`` (int32 [hypotheses]) and ``models`` (float32 [hypotheses, 9]) every hypothesis
    when given.  ``workspace``: int64 or uint64 CUDA tensor of at least ``_native.epipolar_workspace_bytes(n, hypotheses) / 8`` elements,
    no initialisation needed.  Four launches on ``stream`` (a torch.cuda.Stream; default: torch's current stream), no synchronisation, no
    allocation: capturable.  Every argument is checked before the device is touched."""
    args = epipolar_ransac_args(ctx, ref_uv, cur_uv, status, image_size, threshold, hypotheses, seed, workspace, best, n_inliers, F, counts, models, stream)
    N.check(N.lib().ftk_epipolar_ransac_device(*args), ctx.handle)
