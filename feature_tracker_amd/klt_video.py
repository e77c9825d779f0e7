"""``KltVideoTracker``: the sparse trackers over a frame sequence, on a fixed-capacity track table that lives on the device.

A visual-odometry front end runs the same loop on every frame: track the features it has, drop the lost ones, detect new corners that
keep their distance from the survivors, give the new ones identities.  Here that loop is one call per frame and, in the steady state,
a handful of launches on one stream: no copy to the host, no count read back, no synchronisation.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _native as N
from ._device_epipolar import SEED_ARG, check_sizes, epipolar_ransac_args
from ._device_two_view import check_mode, prefer_to_permille, two_view_ransac_args
from ._device_klt_video import harris_survivor_bound, track_table_fill_args, track_table_retire_args
from ._torch_call import OnStream, call, check_ctx
from .track_odometry import TrackOdometry
from .tracker import OUTSIDE, ImagePyramid, OpticalFlow

_MIN_SIDE = 23  # 2 * Harris border + 1: a smaller image has no valid centre


class KltVideoTracker:
    """``tracker.track(image)`` once per frame; afterwards the table is in the attributes, valid until the next call:

    ========== =================== ==========================================
    ids        int64 [N]           -1 = empty
    points     float32 [N, 2]      current frame, (u, v) = (col, row)
    prev_points float32 [N, 2]     previous frame
    status     uint8 [N]           TrackStatus; an empty slot has one above TRACKED
    age        int32 [N]           frames tracked since detection
    n_live     int32 [1]           live slots
    next_id    int64 [1]           the next identity to hand out
    ========== =================== ==========================================

    Slots never move: a slot index is stable for the life of a track, and every launch covers all ``N = max_features`` slots, so no
    count is ever read back.  ``flow`` is an OpticalFlowBasicKlt / OpticalFlowAffineKlt / OpticalFlowLssdKlt; its options, method, prior
    and luminance flag are used as they are at each call.  ``forward_backward=t`` adds a second tracker call in the opposite direction
    and retires a track whose round trip ends more than ``t`` pixels from where it started.  ``epipolar_threshold=t`` adds two-view outlier
    rejection (``EpipolarRansac``) on the forward results, before the backward call (which then skips the rejected slots)
    and before retire: a track more than ``t`` pixels (Sampson) from the best of ``epipolar_hypotheses`` fundamental matrices retires with
    LARGE_RESIDUAL.  The seed of frame f (counted from construction or ``reset()``, the first frame is 0) is ``epipolar_seed + f``, a host
    integer; ``epipolar_F`` / ``epipolar_n_inliers`` / ``epipolar_best`` hold the last fit
    (zeros, 0 and -1 before the first one and after ``reset()``).  None: no such launch.  ``epipolar_model="homography"`` or ``"auto"``
    routes the same step through ``TwoViewRansac`` (``epipolar_prefer_homography`` is its ``prefer_homography``):
    ``epipolar_F`` / ``epipolar_H`` float32 [3, 3], ``epipolar_n_inliers`` / ``epipolar_best`` int32 [2] (slot 0 the fundamental matrix,
    slot 1 the homography) and ``epipolar_model_chosen`` int32 [1] (-1 before the first fit) then hold the last fit; with the default
    ``"fundamental"`` the tracker launches what it launches without the argument and the two new attributes stay None.
    ``odometry``: a ``TrackOdometry`` built on the same ``ctx`` (anything else is a ValueError at construction); ``track()`` then ends with
    ``odometry.update(self.ids, self.points, (H, W))``, after the fill; ``reset()`` of the tracker leaves it alone.  None: the
    tracker launches exactly what it launches without the argument.  ``ctx``: a context made by
    ``device.context_on_stream`` (torch must know the stream the kernels run on); None: the tracker makes a stream and a context of its own.

    Limits: uint8 images of at least 23 x 23 and of one shape (``reset()`` before another), float32 points, the context's stream (the
    caller's current torch stream waits for it, on the device, at the end of every call), no CPU fallback, not promised capturable (the
    tracker entry may grow the context's scratch), no motion prediction (every track starts its search where it was)."""

    def __init__(self, flow, max_features: int, levels: int = 4, min_distance: int = 25, min_response: float = 40.0,
                 forward_backward: Optional[float] = None, ctx=None, epipolar_threshold: Optional[float] = None, epipolar_hypotheses: int = 512,
                 epipolar_seed: int = 0, epipolar_model: str = "fundamental", epipolar_prefer_homography: float = 0.75, odometry=None):
        if not isinstance(flow, OpticalFlow) or flow._model is None:
            raise ValueError(f"flow must be an OpticalFlowBasicKlt, OpticalFlowAffineKlt or OpticalFlowLssdKlt (got {type(flow).__name__})")
        n = int(max_features)
        if not 1 <= n <= N.FTK_TRACK_TABLE_MAX_SLOTS:
            raise ValueError(f"max_features must be in 1 .. {N.FTK_TRACK_TABLE_MAX_SLOTS} (got {max_features})")
        if n > int(flow.options().kMaxTrackPointsNumber):
            raise ValueError(f"max_features {n} exceeds flow.options().kMaxTrackPointsNumber = {int(flow.options().kMaxTrackPointsNumber)}: "
                             "the tracker would leave the slots beyond it untouched")
        if not 1 <= int(levels) <= N.FTK_MAX_LEVELS:
            raise ValueError(f"levels must be in 1 .. {N.FTK_MAX_LEVELS} (got {levels})")
        if int(min_distance) < 1:
            raise ValueError(f"min_distance must be at least 1 (got {min_distance})")
        if forward_backward is not None and not float(forward_backward) >= 0.0:
            raise ValueError(f"forward_backward must be None or a threshold in pixels >= 0 (got {forward_backward})")
        self.epipolar_threshold = None
        self.epipolar_model = "fundamental"
        if epipolar_threshold is None and epipolar_model != "fundamental":
            raise ValueError(f"epipolar_model={epipolar_model!r} needs epipolar_threshold: without a threshold no filter runs")
        if epipolar_threshold is not None:
            if not isinstance(epipolar_model, str):
                raise ValueError(f"epipolar_model must be 'fundamental', 'homography' or 'auto' (got {epipolar_model!r})")
            self._epipolar_mode = check_mode(epipolar_model)
            self.epipolar_model = epipolar_model
            self._epipolar_permille = prefer_to_permille(epipolar_prefer_homography)
            _, _, self.epipolar_threshold, self.epipolar_hypotheses, self.epipolar_seed = check_sizes((1, 1), epipolar_threshold, epipolar_hypotheses,
                                                                                                      epipolar_seed)
        check_ctx(ctx, none_means="the tracker makes its own", because="the table's tensors are torch's, and ")
        if odometry is not None:
            if not isinstance(odometry, TrackOdometry):
                raise ValueError(f"odometry must be a TrackOdometry or None (got {type(odometry).__name__})")
            if ctx is None or odometry._ctx is not ctx:
                raise ValueError("odometry must be a TrackOdometry built on this tracker's ctx (device.context_on_stream): its launches follow the "
                                 "tracker's on one stream of one device")
        self.odometry = odometry
        self.flow, self.max_features, self.levels = flow, n, int(levels)
        self.min_distance, self.min_response = int(min_distance), float(min_response)
        self.forward_backward = None if forward_backward is None else float(forward_backward)
        self._ctx = ctx
        self._shape = None
        self._pyramids = None
        self._frames = 0
        self._spare = 0
        self._image = None
        self.ids = self.points = self.prev_points = self.status = self.age = self.n_live = self.next_id = None
        self.epipolar_F = self.epipolar_n_inliers = self.epipolar_best = None
        self.epipolar_H = self.epipolar_model_chosen = None

    # ---- the caller's side ------------------------------------------------------------------------------------------------------

    def reset(self) -> "KltVideoTracker":
        """Empties the table; identities go on from ``next_id``.  The next frame may have another shape."""
        self._frames = 0
        self._shape = None
        self._pyramids = None
        self._image = None
        if self.ids is not None:
            with OnStream(self._ctx, self.ids):
                self._empty_table()
        return self

    def live(self):
        """(ids, points, prev_points, age) of the live slots, by boolean indexing: the one place that synchronises."""
        if self.ids is None:
            raise RuntimeError("KltVideoTracker.live() before the first track()")
        keep = self.ids >= 0
        return self.ids[keep], self.points[keep], self.prev_points[keep], self.age[keep]

    def track(self, image) -> "KltVideoTracker":
        """The next frame: uint8 [H, W], a CUDA tensor (read in place, stream-ordered) or a C-contiguous numpy array (uploaded).  Builds its
        pyramid, tracks every live slot from the previous frame (not on the first frame after construction or ``reset()``), retires the
        lost ones, detects corners that keep ``min_distance`` from the survivors and fills the empty slots with them.  Returns self."""
        host, rows, cols = self._check_image(image)
        n = self.max_features
        if n > int(self.flow.options().kMaxTrackPointsNumber):
            raise ValueError(f"max_features {n} exceeds flow.options().kMaxTrackPointsNumber = {int(self.flow.options().kMaxTrackPointsNumber)}")
        from . import device as D

        torch = self._torch = D._torch()
        if self._ctx is None:
            self._ctx = D.context_on_stream(torch.cuda.Stream(image.device if not host else None))
        ctx = self._ctx
        device = torch.device("cuda", ctx.device_index)
        if not host and image.device != device:
            raise ValueError(f"image must be on {device}, the context's device (got one on {image.device})")
        with OnStream(ctx, device):
            if self.ids is None:
                self._allocate(device)
            if self._pyramids is None:
                blank = np.zeros((rows, cols), dtype=np.uint8)
                self._pyramids = [ImagePyramid.build(blank, self.levels, ctx), ImagePyramid.build(blank, self.levels, ctx)]
                self._shape = (rows, cols)
                self._bound = {}
            cur, prev = self._pyramids[self._spare], self._pyramids[1 - self._spare]
            if host:
                cur.update(image, "host")
            else:
                self._image = image  # read by the pyramid launch after this call returns
                cur.update(int(image.data_ptr()), "device")
            if self._frames > 0:
                self._track_and_retire(D, prev, cur)
            fill = self._bound.get(("fill", self._spare))
            if fill is None:
                fill = self._bound[("fill", self._spare)] = track_table_fill_args(
                    ctx, cur, self.min_distance, self.min_response, self.ids, self.points, self.prev_points, self.status, self.age, self.n_live, self.next_id,
                    self._free, self._n_free)
            call("ftk_track_table_fill_device", fill, ctx)
            if self.odometry is not None:
                self.odometry.update(self.ids, self.points, self._shape)
        self._spare = 1 - self._spare
        self._frames += 1
        return self

    # ---- inside -----------------------------------------------------------------------------------------------------------------

    def _check_image(self, image):
        """(is a host array, rows, cols), or the ValueError: before anything touches a device."""
        host = isinstance(image, np.ndarray)
        if host:
            if image.dtype != np.uint8 or image.ndim != 2 or not image.flags["C_CONTIGUOUS"]:
                raise ValueError(f"image must be a C-contiguous uint8 [H, W] array (got {image.dtype} {list(image.shape)})")
        else:
            if not hasattr(image, "data_ptr") or str(image.dtype) != "torch.uint8" or image.dim() != 2:
                what = type(image).__name__ if not hasattr(image, "data_ptr") else f"{image.dtype} {list(image.shape)}"
                raise ValueError(f"image must be a uint8 [H, W] CUDA tensor or numpy array (got {what})")
            if not image.is_contiguous():
                raise ValueError(f"image must be contiguous (got strides {list(image.stride())}): nothing is copied here, pass image.contiguous()")
            if not image.is_cuda:
                raise ValueError("image must be a CUDA tensor or a numpy array: a CPU tensor is neither, and there is no CPU fallback")
        rows, cols = (int(e) for e in image.shape)
        if rows < _MIN_SIDE or cols < _MIN_SIDE:
            raise ValueError(f"image must be at least {_MIN_SIDE} x {_MIN_SIDE} (got {rows} x {cols}): a smaller one has no valid Harris centre")
        if self._shape is not None and (rows, cols) != self._shape:
            raise ValueError(f"image is {rows} x {cols} but the sequence so far is {self._shape[0]} x {self._shape[1]}: call reset() before a sequence "
                             "of another shape")
        bound = harris_survivor_bound(rows, cols, self.min_distance)
        if bound > N.FTK_HARRIS_DEVICE_MAX_SURVIVORS:
            raise ValueError(f"a {rows} x {cols} image at min_distance {self.min_distance} can hold {bound} corners, above "
                             f"FTK_HARRIS_DEVICE_MAX_SURVIVORS = {N.FTK_HARRIS_DEVICE_MAX_SURVIVORS}: raise min_distance")
        return host, rows, cols

    def _allocate(self, device):
        torch, n = self._torch, self.max_features
        self.ids = torch.empty(n, dtype=torch.int64, device=device)
        self.points = torch.empty((n, 2), dtype=torch.float32, device=device)
        self.prev_points = torch.empty((n, 2), dtype=torch.float32, device=device)
        self.status = torch.empty(n, dtype=torch.uint8, device=device)
        self.age = torch.empty(n, dtype=torch.int32, device=device)
        self.n_live = torch.empty(1, dtype=torch.int32, device=device)
        self.next_id = torch.zeros(1, dtype=torch.int64, device=device)
        self._free = torch.empty(n, dtype=torch.int32, device=device)
        self._n_free = torch.empty(1, dtype=torch.int32, device=device)
        # the tracker calls' results (forward, backward): separate from the table, which retire moves on
        self._uv = [torch.zeros((n, 2), dtype=torch.float32, device=device) for _ in range(2)]
        self._st = [torch.zeros(n, dtype=torch.uint8, device=device) for _ in range(2)]
        if self.epipolar_threshold is not None:
            # the model decides, once: the number of slots of the outputs, the args builder, the entry, and what follows the seed in its arguments
            two = self.epipolar_model != "fundamental"  # the homography, or the choice between the two
            slots = 2 if two else 1
            bytes_ = N.two_view_workspace_bytes(n, self.epipolar_hypotheses, self._epipolar_mode) if two else N.epipolar_workspace_bytes(n, self.epipolar_hypotheses)
            self._epipolar_ws = torch.empty(-(-bytes_ // 8), dtype=torch.int64, device=device)
            self.epipolar_F = torch.zeros((3, 3), dtype=torch.float32, device=device)
            self.epipolar_n_inliers = torch.zeros(slots, dtype=torch.int32, device=device)
            self.epipolar_best = torch.full((slots,), -1, dtype=torch.int32, device=device)
            if two:
                self.epipolar_H = torch.zeros((3, 3), dtype=torch.float32, device=device)
                self.epipolar_model_chosen = torch.full((1,), -1, dtype=torch.int32, device=device)
                self._epipolar_call = ("two_view", two_view_ransac_args, "ftk_two_view_ransac_device", (
                    self._epipolar_mode, self._epipolar_permille, self._epipolar_ws, self.epipolar_model_chosen, self.epipolar_best, self.epipolar_n_inliers,
                    self.epipolar_F, self.epipolar_H))
            else:
                self._epipolar_call = ("epipolar", epipolar_ransac_args, "ftk_epipolar_ransac_device", (
                    self._epipolar_ws, self.epipolar_best, self.epipolar_n_inliers, self.epipolar_F))
        self._empty_table()

    def _empty_table(self):
        torch, n = self._torch, self.max_features
        self.ids.fill_(-1)
        self.points.zero_()
        self.prev_points.zero_()
        self.status.fill_(OUTSIDE)
        self.age.zero_()
        self.n_live.zero_()
        self._free.copy_(torch.arange(n, dtype=torch.int32, device=self.ids.device))
        if self.epipolar_F is not None:  # no fit yet: the first frame of a sequence runs no filter
            self.epipolar_F.zero_()
            self.epipolar_n_inliers.zero_()
            self.epipolar_best.fill_(-1)
        if self.epipolar_H is not None:
            self.epipolar_H.zero_()
            self.epipolar_model_chosen.fill_(-1)
        self._n_free.fill_(n)

    def _track_and_retire(self, D, prev, cur):
        flow, ctx = self.flow, self._ctx
        prior, lum = flow._prior(), flow._luminance()
        D.DeviceKlt(_MODEL_NAMES[flow._model], flow.options(), prev, cur, ctx, prior, lum).track(self.points, self.points, self.status, self._uv[0], self._st[0])
        if self.epipolar_threshold is not None:
            self._reject_outliers()
        fb = self.forward_backward is not None
        if fb:
            D.DeviceKlt(_MODEL_NAMES[flow._model], flow.options(), cur, prev, ctx, prior, lum).track(self._uv[0], self._uv[0], self._st[0], self._uv[1], self._st[1])
        retire = self._bound.get("retire")
        if retire is None:
            retire = self._bound["retire"] = track_table_retire_args(
                ctx, self.ids, self.points, self.prev_points, self.status, self.age, self.n_live, self._uv[0], self._st[0], self._free, self._n_free,
                self._uv[1] if fb else None, self._st[1] if fb else None, self.forward_backward if fb else 0.0)
        call("ftk_track_table_retire_device", retire, ctx)

    def _reject_outliers(self):
        """The forward results against the best fundamental matrix (or the chosen model): ``_st[0]`` of a tracked slot that disagrees becomes LARGE_RESIDUAL."""
        ctx = self._ctx
        key, marshal, entry, rest = self._epipolar_call
        args = self._bound.get(key)
        if args is None:
            args = self._bound[key] = list(marshal(ctx, self.points, self._uv[0], self._st[0], self._shape, self.epipolar_threshold, self.epipolar_hypotheses, 0,
                                                   *rest, stream=ctx.stream))
        args[SEED_ARG] = C.c_uint32((self.epipolar_seed + self._frames) & 0xFFFFFFFF)
        call(entry, args, ctx)


_MODEL_NAMES = {v: k for k, v in N.MODELS.items()}
