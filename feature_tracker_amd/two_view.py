"""``TwoViewRansac``: two-view outlier rejection with a choice of model on the device.

``EpipolarRansac``'s fundamental matrix constrains only a scene with parallax; on a plane, or from a camera that does not move, every
motion fits some fundamental matrix.  The standard answer is a second model, a homography, fitted by the same RANSAC, and a rule that
picks the model the data support.  Here that is four launches for one model and six for both, on one stream, on tensors that stay where
they are: no copy to the host, no count read back, no synchronisation.
"""
from __future__ import annotations

from typing import Optional

from . import _native as N
from ._device_epipolar import check_sizes
from ._device_two_view import check_mode, prefer_to_permille, two_view_ransac_args
from ._torch_call import PerDevice, check_ctx
from .epipolar import ransac_filter


class TwoViewResult:
    """What one ``filter`` call leaves, all on the device: ``model`` int32 [1] (0: the fundamental matrix was applied, 1: the homography, -1:
    nothing changed), ``F`` and ``H`` float32 [3, 3] (pixel units, ``x_cur^T F x_ref = 0`` and ``x_cur ~ H x_ref``; zeros when the model did
    not run or has no winner), ``n_inliers`` and ``best`` int32 [2] (slot 0 the fundamental matrix, slot 1 the homography; M and -1 without a
    winner), and, when asked for, ``counts`` int32 [2, K] (-1: an invalid hypothesis) and ``models`` float32 [2, K, 9] (normalised)."""

    __slots__ = ("model", "F", "H", "n_inliers", "best", "counts", "models")

    def __init__(self, model, F, H, n_inliers, best, counts=None, models=None):
        self.model, self.F, self.H, self.n_inliers, self.best, self.counts, self.models = model, F, H, n_inliers, best, counts, models


class TwoViewRansac:
    """``TwoViewRansac(model="auto", hypotheses=512, threshold=1.0, prefer_homography=0.75, seed=0).filter(ref_uv, cur_uv, status, image_size)``.

    The arguments of ``filter``, the participants, the normalisation, the sampler and the limits are ``EpipolarRansac``'s.  ``model``:
    "fundamental" computes what ``EpipolarRansac`` computes, bit for bit; "homography" fits ``x_cur ~ H x_ref`` from 4 correspondences per
    hypothesis (the 8 x 9 DLT system, the same elimination) and counts a point as an inlier when its one-sided transfer error in the
    current image is at most ``threshold`` pixels; "auto" runs both on the same participants and seed and applies the homography iff it
    has a winner and (the fundamental matrix has none, or ``1000 n_H >= round(1000 prefer_homography) n_F``), else the fundamental matrix.
    The default 0.75 is a design default, not a measured optimum: a homography that explains three quarters of what the fundamental matrix
    explains tolerates up to a quarter of the points on independently moving objects, and keeps the fundamental matrix where a dominant
    plane leaves more than a quarter of the points off the plane.  Only the chosen model's non-inliers become LARGE_RESIDUAL.  With 4 .. 7
    participants "auto" can only choose the homography; with fewer than 4 nothing changes.

    Out of scope: the symmetric transfer error, an orientation (cheirality) test and a refit on the inliers; ``H`` is for rejecting
    outliers.  Stream handling, workspace policy and capturability are ``EpipolarRansac``'s."""

    def __init__(self, model: str = "auto", hypotheses: int = 512, threshold: float = 1.0, prefer_homography: float = 0.75, seed: int = 0, ctx=None):
        self.mode = check_mode(model)
        self.model = model
        self.prefer_homography_permille = prefer_to_permille(prefer_homography)
        _, _, self.threshold, self.hypotheses, self.seed = check_sizes((1, 1), threshold, hypotheses, seed)
        check_ctx(ctx)
        self._ctx = ctx
        self._workspace = PerDevice()  # device -> the one workspace of this object on it, grown to the largest call so far

    def filter(self, ref_uv, cur_uv, status, image_size, seed: Optional[int] = None, return_hypotheses: bool = False) -> TwoViewResult:
        """One pass of outlier rejection; ``seed``: this call's seed instead of the object's; ``return_hypotheses``: also ``counts`` and
        ``models``.  Everything is enqueued; the returned tensors are valid in stream order."""
        return ransac_filter(self, ref_uv, cur_uv, status, image_size, seed, return_hypotheses)

    _entry = "ftk_two_view_ransac_device"

    def _workspace_bytes(self, n, k):
        return N.two_view_workspace_bytes(n, k, self.mode)

    def _result(self, torch, device, k, return_hypotheses):
        i32 = dict(dtype=torch.int32, device=device)
        f32 = dict(dtype=torch.float32, device=device)
        out = TwoViewResult(torch.empty(1, **i32), torch.empty((3, 3), **f32), torch.empty((3, 3), **f32), torch.empty(2, **i32), torch.empty(2, **i32))
        if return_hypotheses:
            out.counts = torch.empty((2, k), **i32)
            out.models = torch.empty((2, k, 9), **f32)
        return out

    def _args(self, ctx, ref_uv, cur_uv, status, image_size, k, seed, workspace, out, stream):
        return two_view_ransac_args(ctx, ref_uv, cur_uv, status, image_size, self.threshold, k, seed, self.mode, self.prefer_homography_permille,
                                    workspace, out.model, out.best, out.n_inliers, out.F, out.H, out.counts, out.models, stream)
