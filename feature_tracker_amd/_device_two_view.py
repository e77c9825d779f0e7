"""``device.two_view_ransac_device``: the torch device entry of two-view outlier rejection with a choice of model
(ftk_two_view_ransac_device).

It is re-exported by device.py and held to that module's rule: no ``datapointer()`` of a tensor that did not pass ``device._check``.  It lives
in a file of its own for _device_epipolar.py's reason; its walk and its refusals are tests/test_two_view_args_cpu.py.
"""
from __future__ import annotations

import math

from . import _native as N
from ._torch_call import pointer
from ._device_epipolar import SEED_ARG, check_sizes, ransac_inputs  # noqa: F401  (SEED_ARG: both entries share the arguments up to the seed)


def check_mode(model) -> int:
    """The mode the ABI takes for a model's name (or its number), or the ValueError."""
    if isinstance(model, str) and model in N.TWO_VIEW_MODES:
        return N.TWO_VIEW_MODES[model]
    if isinstance(model, int) and not isinstance(model, bool) and model in N.TWO_VIEW_MODES.values():
        return model
    raise ValueError(f"model must be one of {sorted(N.TWO_VIEW_MODES)} (got {model!r})")


def check_permille(permille) -> int:
    if isinstance(permille, bool) or not isinstance(permille, int) or not 0 <= permille <= 1000:
        raise ValueError(f"prefer_homography_permille must be an integer in 0 .. 1000 (got {permille!r})")
    return permille


def prefer_to_permille(prefer_homography) -> int:
    """``round(1000 x)`` of a finite x in [0, 1], or the ValueError."""
    try:
        x = float(prefer_homography)
    except (TypeError, ValueError):
        x = math.nan
    if not (math.isfinite(x) and 0.0 <= x <= 1.0):
        raise ValueError(f"prefer_homography must be a finite number in [0, 1] (got {prefer_homography!r})")
    return int(round(1000.0 * x))


def two_view_ransac_args(ctx, ref_uv, cur_uv, status, image_size, threshold: float, hypotheses: int, seed: int, model, prefer_homography_permille: int,
                         workspace, model_out, best, n_inliers, F, H, counts=None, models=None, stream=None):
    """Checks one ftk_two_view_ransac_device call and returns its marshalled arguments (KltVideoTracker keeps them: its tensors are fixed)."""
    sizes = check_sizes(image_size, threshold, hypotheses, seed)
    mode, permille = check_mode(model), check_permille(prefer_homography_permille)
    D, dev, n, k, head = ransac_inputs(ctx, ref_uv, cur_uv, status, sizes, stream)
    D._check("workspace", workspace, D._KEYS, (None,), dev, min_numel=-(-N.two_view_workspace_bytes(n, k, mode) // 8))
    D._check("model_out", model_out, D._I32, (1,), dev)
    D._check("best", best, D._I32, (2,), dev)
    D._check("n_inliers", n_inliers, D._I32, (2,), dev)
    D._check("F", F, D._F32, (3, 3), dev)
    D._check("H", H, D._F32, (3, 3), dev)
    if counts is not None:
        D._check("counts", counts, D._I32, (2, k), dev)
    if models is not None:
        D._check("models", models, D._F32, (2, k, 9), dev)
    return head + (mode, permille, pointer(workspace), pointer(model_out), pointer(best), pointer(n_inliers), pointer(F), pointer(H), pointer(counts), pointer(models))


def two_view_ransac_device(ctx, ref_uv, cur_uv, status, image_size, threshold: float, hypotheses: int, seed: int, model, prefer_homography_permille: int,
                           workspace, model_out, best, n_inliers, F, H, counts=None, models=None, stream=None) -> None:
    """ftk_two_view_ransac_device: RANSAC on the fundamental matrix (``model`` "fundamental" or 0), on a homography ("homography", 1) or on
    both with the rule of DESIGN.md 5.21 ("auto", 2; the homography is chosen iff it has a winner and the fundamental matrix has none or
    ``1000 n_H >= prefer_homography_permille n_F``), over the correspondences ``ref_uv[i] -> cur_uv[i]`` (contiguous float32 CUDA [n, 2])
    whose ``status`` (uint8 [n]) is TRACKED; ``status`` is rewritten in place (a participant that is no inlier of the chosen model becomes
    LARGE_RESIDUAL).  ``model_out`` int32 [1] receives -1, 0 or 1; ``best`` / ``n_inliers`` int32 [2], ``F`` / ``H`` float32 [3, 3] (pixel
    units) the winner of each model (slot 0 the fundamental matrix, slot 1 the homography); ``counts`` int32 [2, hypotheses] and ``models``
    float32 [2, hypotheses, 9] every hypothesis when given.  ``workspace``: int64 or uint64 CUDA tensor of at least
    ``_native.two_view_workspace_bytes(n, hypotheses) / 8`` elements.  Four launches (six with "auto") on ``stream`` (default: torch's current
    stream), no synchronisation, no allocation: capturable.  Every argument is checked before the device is touched."""
    args = two_view_ransac_args(ctx, ref_uv, cur_uv, status, image_size, threshold, hypotheses, seed, model, prefer_homography_permille, workspace,
                                model_out, best, n_inliers, F, H, counts, models, stream)
    N.check(N.lib().ftk_two_view_ransac_device(*args), ctx.handle)
