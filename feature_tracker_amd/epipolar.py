"""``EpipolarRansac``: two-view outlier rejection on the device.

Geometric verification is what every visual-odometry front end runs right after tracking or matching: fit a fundamental matrix by RANSAC
and drop the correspondences that disagree with it.  Here that is four launches of two_view_kernels.hip on one stream, on tensors that
stay where they are: no copy to the host, no count read back, no synchronisation.
"""
from __future__ import annotations

from typing import Optional

from . import _native as N
from ._device_epipolar import check_sizes, epipolar_ransac_args
from ._torch_call import OnStream, PerDevice, call, check_ctx, complain


def ransac_filter(ransac, ref_uv, cur_uv, status, image_size, seed, return_hypotheses):
    """``EpipolarRansac.filter`` and ``TwoViewRansac.filter``: the complaints about the tensors, the choice of context and stream, the one
    workspace per device of ``ransac`` and the call.  ``ransac`` says what differs: ``_workspace_bytes(n, k)``, ``_result(torch, device, k,
    return_hypotheses)`` (the result object with its tensors), ``_args(ctx, ..., workspace, out, stream)`` (the marshalled arguments) and
    ``_entry`` (the native entry they are for)."""
    rows, cols, _, k, seed = check_sizes(image_size, ransac.threshold, ransac.hypotheses, ransac.seed if seed is None else seed)
    from . import device as D

    tensors = (("ref_uv", ref_uv, D._F32, (None, 2)), ("cur_uv", cur_uv, D._F32, (None, 2)), ("status", status, D._U8, (None,)))
    complain(tensors)
    device, n = ref_uv.device, int(ref_uv.shape[0])
    with OnStream(ransac._ctx, ref_uv) as on:
        workspace = ransac._workspace.get(device)  # (of an n outside the limits: whatever there is, and the entry's refusal)
        if 1 <= n <= N.FTK_TRACK_TABLE_MAX_SLOTS:
            workspace = ransac._workspace.of(on.torch, device, ransac._workspace_bytes(n, k))
        out = ransac._result(on.torch, device, k, return_hypotheses)
        call(ransac._entry, ransac._args(on.ctx, ref_uv, cur_uv, status, (rows, cols), k, seed, workspace, out, on.stream), on.ctx)
    return out


class EpipolarResult:
    """What one ``filter`` call leaves, all on the device: ``F`` float32 [3, 3] (pixel units, ``x_cur^T F x_ref = 0``; zeros when there is no
    model), ``n_inliers`` int32 [1], ``best`` int32 [1] (the winning hypothesis, -1: none), and, when asked for, ``counts`` int32 [K] (-1: an
    invalid hypothesis) and ``models`` float32 [K, 9] (the normalised F of every hypothesis)."""

    __slots__ = ("F", "n_inliers", "best", "counts", "models")

    def __init__(self, F, n_inliers, best, counts=None, models=None):
        self.F, self.n_inliers, self.best, self.counts, self.models = F, n_inliers, best, counts, models


class EpipolarRansac:
    """``EpipolarRansac(hypotheses=512, threshold=1.0, seed=0).filter(ref_uv, cur_uv, status, image_size)``.

    ``ref_uv`` / ``cur_uv``: contiguous float32 CUDA [N, 2], (u, v) pixels; ``status``: uint8 CUDA [N], rewritten IN PLACE.  The points whose
    status is TRACKED take part; one that is not an inlier of the winning fundamental matrix (Sampson distance above ``threshold`` pixels)
    becomes LARGE_RESIDUAL; every other point keeps its status.  With fewer than 8 participants, or no valid hypothesis, nothing changes
    and ``best`` is -1.  The result is a pure function of the inputs and the seed (integer counts, integer atomics: no run-to-run variation).

    The model is the 8-point null vector of each sample by Gaussian elimination with complete pivoting in float32: no rank-2 projection and
    no refit on the inliers (DESIGN.md 5.20 says why), so ``F`` is for rejecting outliers, not for recovering a pose.

    ``ctx``: a context made by ``device.context_on_stream`` (the call runs on its stream, which waits for torch's current stream and is
    waited for by it, on the device); None: a context of the tensors' device, and the
    call runs on torch's current stream.  Limits: N in 1 .. 65 536, hypotheses in 1 .. 4 096, no CPU fallback.  Capturable in
    ``torch.cuda.graph`` (nothing is read back, nothing synchronises; the tensors it makes come from torch's allocator) after one call of
    at least the size outside the capture.  The object keeps ONE workspace per device, grown by a quarter beyond the largest call so far, so
    a caller whose N changes from call to call does not accumulate blocks; calls on one object are therefore ordered on one stream — use one
    object per stream that runs concurrently."""

    def __init__(self, hypotheses: int = 512, threshold: float = 1.0, seed: int = 0, ctx=None):
        _, _, self.threshold, self.hypotheses, self.seed = check_sizes((1, 1), threshold, hypotheses, seed)
        check_ctx(ctx)
        self._ctx = ctx
        self._workspace = PerDevice()  # device -> the one workspace of this object on it, grown to the largest call so far

    def filter(self, ref_uv, cur_uv, status, image_size, seed: Optional[int] = None, return_hypotheses: bool = False) -> EpipolarResult:
        """One pass of outlier rejection; ``seed``: this call's seed instead of the object's; ``return_hypotheses``: also ``counts`` and
        ``models``.  Everything is enqueued; the returned tensors are valid in stream order."""
        return ransac_filter(self, ref_uv, cur_uv, status, image_size, seed, return_hypotheses)

    _entry = "ftk_epipolar_ransac_device"

    def _workspace_bytes(self, n, k):
        return N.epipolar_workspace_bytes(n, k)

    def _result(self, torch, device, k, return_hypotheses):
        out = EpipolarResult(torch.empty((3, 3), dtype=torch.float32, device=device), torch.empty(1, dtype=torch.int32, device=device),
                             torch.empty(1, dtype=torch.int32, device=device))
        if return_hypotheses:
            out.counts = torch.empty(k, dtype=torch.int32, device=device)
            out.models = torch.empty((k, 9), dtype=torch.float32, device=device)
        return out

    def _args(self, ctx, ref_uv, cur_uv, status, image_size, k, seed, workspace, out, stream):
        return epipolar_ransac_args(ctx, ref_uv, cur_uv, status, image_size, self.threshold, k, seed, workspace, out.best, out.n_inliers, out.F,
                                    out.counts, out.models, stream)
