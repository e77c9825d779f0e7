"""``PnpRansac``: the pose of the camera from landmarks and the pixels where they are seen, on the device.

``TwoViewPose`` turns the first two views into a pose and landmarks; ``DirectMethod`` refines a pose once it has one.  This is what every
frame after the second asks in between: given the landmarks there are and the pixels where their tracks are now, where is the camera?
RANSAC over the six-point DLT or over P3P (``sample``), then a Gauss-Newton refit of the reprojection error on the inliers; 5 + 2
``refine_iterations`` launches on one stream, on tensors that stay where they are: no copy to the host, no count read back, no synchronisation.
"""
from __future__ import annotations

from typing import Optional

from . import _native as N
from ._device_pnp import check_counts, check_sample, pnp_args
from ._device_two_view_pose import check_camera, check_scalars
from ._torch_call import OnStream, PerDevice, call, check_ctx, complain


class PnpResult:
    """What one ``solve`` call leaves, all on the device: ``pose`` float32 [7] (q_rc as (w, x, y, z) with w >= 0, then p_rc: DirectMethod's
    convention, ``x_cur ~ q_rc^-1 (X - p_rc)``), ``n_inliers`` int32 [1] (the participants that keep TRACKED), ``best`` int32 [1] (the
    winning hypothesis, -1: none), ``valid`` int32 [1] (1, or -1: nothing changed, identity pose, no inliers), and, when asked for,
    ``counts`` int32 [K] (-1: an invalid hypothesis) and ``models`` float32 [K, 12] (every hypothesis' [A | b], row-major; under
    ``sample="p3p"`` it is [R | t])."""

    __slots__ = ("pose", "n_inliers", "best", "valid", "counts", "models")

    def __init__(self, pose, n_inliers, best, valid, counts=None, models=None):
        self.pose, self.n_inliers, self.best, self.valid, self.counts, self.models = pose, n_inliers, best, valid, counts, models


class PnpRansac:
    """``PnpRansac(K, hypotheses=512, threshold=1.0, refine_iterations=4, seed=0, ctx=None, sample="dlt6").solve(landmarks, uv, status)``.

    ``K``: (fx, fy, cx, cy).  ``landmarks``: contiguous float32 CUDA [N, 3], points in the frame ``TwoViewPose``'s ``points`` are in;
    ``uv``: float32 CUDA [N, 2], (u, v) pixels; ``status``: uint8 CUDA [N], rewritten IN PLACE.  A row takes part iff its status is
    TRACKED, its five numbers are finite and its landmark is not exactly (0, 0, 0): that is how ``TwoViewPose`` writes "no landmark", so
    its ``points`` and a tracker's table go in unchanged.  A participant keeps TRACKED iff, under the final pose, it lies in front of the
    camera and its reprojection error is at most ``threshold`` pixels; otherwise it becomes LARGE_RESIDUAL.  No other row is touched.
    With fewer participants than a sample (6, or 4 under "p3p"), no valid hypothesis or a non-finite pose the result is invalid:
    ``valid`` -1, the identity pose, no status changed.

    ``sample``: the minimal solver behind the hypotheses.  "dlt6" (the default) is the six-point DLT: it has no unique solution for
    landmarks of one plane, so a planar set gives ``valid`` -1.  "p3p"  draws four participants, solves P3P on the first
    three (Grunert's quartic, float32, a fixed count of Newton steps) and lets the fourth choose among the up to four poses: a planar set
    gives a pose, and a model is a rotation and a translation by construction.  A refit step needs six rows under either: with 4 or 5
    participants the pose is the winning hypothesis'.  Any other value is a ValueError.

    The result is a pure function of the inputs and the seed: integer counts, sums in a fixed tree, a Jacobi with a fixed sweep count.
    Out of scope: EPnP, a robust kernel, a batch dimension.

    ``ctx``, the stream, the one grown workspace per device and capturability (after one call of at least the size) are
    ``EpipolarRansac``'s.  Limits: N in 1 .. 65 536, hypotheses in 1 .. 4 096, refine_iterations in 0 .. 16, no CPU fallback."""

    def __init__(self, K, hypotheses: int = 512, threshold: float = 1.0, refine_iterations: int = 4, seed: int = 0, ctx=None, sample: str = "dlt6"):
        self.sample = check_sample(sample)
        self.K = check_camera("K", K)
        self.threshold, _ = check_scalars(threshold, 1.0)
        self.hypotheses, self.refine_iterations, self.seed = check_counts(hypotheses, refine_iterations, seed)
        check_ctx(ctx)
        self._ctx = ctx
        self._workspace = PerDevice()  # device -> the one workspace of this object on it, grown to the largest call so far

    def solve(self, landmarks, uv, status, seed: Optional[int] = None, return_hypotheses: bool = False) -> PnpResult:
        """One pose.  ``seed``: this call's seed instead of the object's; ``return_hypotheses``: also ``counts`` and ``models``.
        Everything is enqueued; the returned tensors are valid in stream order."""
        from . import device as D

        k, r, seed = check_counts(self.hypotheses, self.refine_iterations, self.seed if seed is None else seed)
        complain((("landmarks", landmarks, D._F32, (None, 3)), ("uv", uv, D._F32, (None, 2)), ("status", status, D._U8, (None,))))
        device, n = landmarks.device, int(landmarks.shape[0])
        with OnStream(self._ctx, landmarks) as on:
            torch = on.torch
            workspace = self._workspace.get(device)  # (of an n outside the limits: whatever there is, and the entry's refusal)
            if 1 <= n <= N.FTK_TRACK_TABLE_MAX_SLOTS:
                workspace = self._workspace.of(torch, device, N.pnp_ransac_workspace_bytes(n, k, r))
            i32, f32 = dict(dtype=torch.int32, device=device), dict(dtype=torch.float32, device=device)
            out = PnpResult(torch.empty(7, **f32), torch.empty(1, **i32), torch.empty(1, **i32), torch.empty(1, **i32))
            if return_hypotheses:
                out.counts, out.models = torch.empty(k, **i32), torch.empty((k, N.FTK_PNP_MODEL_FLOATS), **f32)
            sampled = self.sample != "dlt6"  # ("dlt6" launches what it always has, through the entry it always has)
            call("ftk_pnp_ransac_sampled_device" if sampled else "ftk_pnp_ransac_device",
                 pnp_args(on.ctx, landmarks, uv, status, self.K, self.threshold, k, r, seed, workspace, out.pose, out.n_inliers, out.best, out.valid,
                          out.counts, out.models, on.stream, sample=self.sample if sampled else None), on.ctx)
        return out
