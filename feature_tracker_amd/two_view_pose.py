"""``TwoViewPose``: the relative pose of two views and the landmarks of their inliers on the device.

``EpipolarRansac`` and ``TwoViewRansac`` reject outliers; ``DirectMethod`` starts from a pose and from points in the reference camera
frame.  This is the step between them, the one every visual-odometry initialiser runs: refit the essential matrix on the inliers,
decompose it, vote the four candidates by cheirality, triangulate.  Five launches on one stream, on tensors that stay where they are: no
copy to the host, no count read back, no synchronisation.
"""
from __future__ import annotations

from . import _native as N
from ._device_two_view_pose import check_camera, check_scalars, two_view_pose_args
from ._torch_call import OnStream, PerDevice, call, check_ctx, complain


class TwoViewPoseResult:
    """What one ``solve`` call leaves, all on the device: ``pose`` float32 [7] (q_rc as (w, x, y, z), then p_rc: DirectMethod's convention,
    ``|p_rc| = baseline``), ``points`` float32 [N, 3] (p_c_in_ref; zeros where there is no landmark), ``E`` float32 [3, 3] (calibrated,
    ``x_cur^T E x_ref = 0``, singular values (1, 1, 0)), ``n_front`` int32 [4] (the cheirality count of each candidate), ``valid`` int32 [1]
    (1, or -1: nothing changed, identity pose, zero E and points) and ``n_points`` int32 [1]."""

    __slots__ = ("pose", "points", "E", "n_front", "valid", "n_points")

    def __init__(self, pose, points, E, n_front, valid, n_points):
        self.pose, self.points, self.E, self.n_front, self.valid, self.n_points = pose, points, E, n_front, valid, n_points


class TwoViewPose:
    """``TwoViewPose(K, K_cur=None, threshold=1.0, baseline=1.0).solve(ref_uv, cur_uv, status)``, after ``TwoViewRansac.filter``.

    ``K`` / ``K_cur``: (fx, fy, cx, cy) of the reference and the current view (None: the same camera).  ``ref_uv`` / ``cur_uv``:
    contiguous float32 CUDA [N, 2], (u, v) pixels; ``status``: uint8 CUDA [N], rewritten IN PLACE.  The points whose status is TRACKED take
    part, all of them: this is a least-squares refit, so run it on what a filter left.  A participant ends with a landmark (its two-ray
    depths positive and its reprojection error in the current image at most ``threshold`` pixels) or as LARGE_RESIDUAL with a zero point.
    The translation of two views has no scale: ``|p_rc|`` is set to ``baseline`` and the points scale with it.

    The result is a pure function of the inputs: the sums run in a fixed tree, the eigen-solver is a cyclic Jacobi with a fixed sweep
    count, the counts are integers.  The eight-point refit is degenerate on one plane and under pure rotation; there
    ``TwoViewRansac("auto")`` chooses the homography (check ``fit.model``), and ``solve`` returns whatever the data give.  Out of scope:
    pose from a homography, a five-point solver, non-linear refinement, a parallax test, a batch dimension.

    ``ctx``, the stream, the one grown workspace per device and capturability (after one call of at least the size) are
    ``EpipolarRansac``'s.  Limits: N in 1 .. 65 536, no CPU fallback."""

    def __init__(self, K, K_cur=None, threshold: float = 1.0, baseline: float = 1.0, ctx=None):
        self.K = check_camera("K", K)
        self.K_cur = None if K_cur is None else check_camera("K_cur", K_cur)
        self.threshold, self.baseline = check_scalars(threshold, baseline)
        check_ctx(ctx)
        self._ctx = ctx
        self._workspace = PerDevice()  # device -> the one workspace of this object on it, grown to the largest call so far

    def solve(self, ref_uv, cur_uv, status) -> TwoViewPoseResult:
        """One pose and its landmarks.  Everything is enqueued; the returned tensors are valid in stream order."""
        from . import device as D

        complain((("ref_uv", ref_uv, D._F32, (None, 2)), ("cur_uv", cur_uv, D._F32, (None, 2)), ("status", status, D._U8, (None,))))
        device, n = ref_uv.device, int(ref_uv.shape[0])
        with OnStream(self._ctx, ref_uv) as on:
            torch = on.torch
            workspace = self._workspace.get(device)  # (of an n outside the limits: whatever there is, and the entry's refusal)
            if 1 <= n <= N.FTK_TRACK_TABLE_MAX_SLOTS:
                workspace = self._workspace.of(torch, device, N.two_view_pose_workspace_bytes(n))
            i32, f32 = dict(dtype=torch.int32, device=device), dict(dtype=torch.float32, device=device)
            out = TwoViewPoseResult(torch.empty(7, **f32), torch.empty((max(n, 0), 3), **f32), torch.empty((3, 3), **f32), torch.empty(4, **i32),
                                    torch.empty(1, **i32), torch.empty(1, **i32))
            call("ftk_two_view_pose_device", two_view_pose_args(on.ctx, ref_uv, cur_uv, status, self.K, self.K_cur, self.threshold, self.baseline, workspace,
                                                                out.pose, out.points, out.E, out.n_front, out.valid, out.n_points, on.stream), on.ctx)
        return out
