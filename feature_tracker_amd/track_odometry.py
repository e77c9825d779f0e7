"""``TrackOdometry``: a pose per frame and landmarks for new tracks over a track table, on the device.

``TwoViewPose`` gives landmarks to the tracks of the first pair; a video tracker retires and refills slots every frame, so after a few
dozen frames ``PnpRansac`` runs out of participants.  This class keeps a landmark table beside the track table: it knows which slot's
landmark belongs to which track, triangulates a track born later from two views whose poses are known, and runs ``PnpRansac`` in between.
In the steady state a frame is 2 + 13 launches on one stream: no copy to the host, no count read back, no synchronisation.
"""
from __future__ import annotations

import ctypes as C

from . import _native as N
from ._device_epipolar import check_sizes
from ._device_landmark_table import (END_FRAME_ARG, END_MODE_ARG, END_MODEL_ARG, END_POSE_ARG, END_STATUS_ARG, END_VALID_ARG, STREAM_ARG, check_parallax,
                                     landmark_begin_args, landmark_end_args)
from ._device_pnp import check_counts, check_sample
from ._device_two_view_pose import check_camera, check_scalars
from ._torch_call import OnStream, call, check_ctx, complain, pointer
from .pnp import PnpRansac
from .two_view import TwoViewRansac
from .two_view_pose import TwoViewPose

_I64 = ("int64",)


def check_min_landmarks(min_landmarks) -> int:
    if isinstance(min_landmarks, bool) or not isinstance(min_landmarks, int) or not 6 <= min_landmarks <= N.FTK_TRACK_TABLE_MAX_SLOTS:
        raise ValueError(f"min_landmarks must be an integer in 6 (PnpRansac's sample) .. FTK_TRACK_TABLE_MAX_SLOTS = {N.FTK_TRACK_TABLE_MAX_SLOTS} "
                         f"(got {min_landmarks!r})")
    return min_landmarks


class TrackOdometry:
    """``TrackOdometry(K, threshold=1.0, min_parallax_deg=1.0, min_landmarks=30, baseline=1.0, hypotheses=512, refine_iterations=4,
    seed=0, ctx=None, pnp_sample="dlt6").update(ids, points, image_size)``, once per frame, on any track table: ``ids`` int64 CUDA [n] (-1 = empty; a slot index is
    stable for the life of a track, an id is never reused) and ``points`` float32 CUDA [n, 2], as ``KltVideoTracker`` and
    ``MatchVideoTracker`` keep them.  Afterwards, all on the device and valid until the next call:

    =========== ================= ==========================================================================================
    pose        float32 [7]       q_rc (w, x, y, z), p_rc of the last valid frame in ``DirectMethod``'s convention; world = the anchor camera
    landmarks   float32 [n, 3]    world frame, by slot; exactly (0, 0, 0) = none: goes into ``PnpRansac.solve`` unchanged
    valid       int32 [1]         1, or -1: this frame's pose was invalid and nothing but ``lost`` changed
    n_landmarks int32 [1]         live slots that hold a landmark
    n_new       int32 [1]         landmarks triangulated by this call
    n_dropped   int32 [1]         landmarks dropped by this call because ``PnpRansac`` found them to be outliers
    n_anchored  int32 [1]         live slots that had an anchor when the call began
    lost        int32 [1]         invalid frames in a row; before ``initialised``: bootstrap attempts in a row that gave no pose
    =========== ================= ==========================================================================================

    ``initialised`` and ``frame`` (the number of calls since construction or ``reset()``) are host values.

    Bootstrap.  The first call anchors every live slot at the identity pose.  Each later call filters (anchor pixel, current pixel) with
    ``TwoViewRansac("auto")``, solves ``TwoViewPose(K, baseline=baseline)`` and triangulates every anchored slot by the table's own rule;
    then the host reads three int32 in one copy, the only host read of the class.  A valid pose with at least ``min_landmarks`` new
    landmarks initialises the map; otherwise the landmarks are zeroed and the pair is tried again next frame from the same anchors (a
    homography chosen by "auto" counts as not yet: DESIGN.md 5.29), and with fewer than ``min_landmarks`` anchored slots left the
    bootstrap starts again from the current frame.  The translation of two views has no scale: the map's is ``baseline``.

    Steady state.  ``PnpRansac.solve(landmarks, points, status, seed=seed + frame)`` between the table's two kernels, with
    ``PnpRansac``'s ``sample=pnp_sample`` ("dlt6", or "p3p": a pose also where the landmarks in view lie on one plane; the bootstrap
    still cannot start on one plane).  A landmark that
    ``PnpRansac`` finds to be an outlier is dropped; a live slot without a landmark is anchored and, once its ray and the anchor's meet at
    ``min_parallax_deg`` or more, triangulated by the two-ray midpoint, kept iff it lies in front of both cameras within ``threshold``
    pixels in both, else anchored again.  A frame whose pose is invalid keeps the previous pose and raises ``lost``; there is no automatic
    re-initialisation: ``reset()`` is the caller's.  ``min_parallax_deg`` and ``min_landmarks`` are design defaults, not measured optima.

    Out of scope: relocalisation, bundle adjustment, multi-view landmark refinement, scale recovery, retiring tracks on PnP outliers, a
    batch dimension, a C++ class.  ``ctx``, the stream and capturability (a steady-state call, after one eager call of the size) are
    ``PnpRansac``'s.  Limits: n in 1 .. 65 536 and fixed until ``reset()``, no CPU fallback."""

    def __init__(self, K, threshold: float = 1.0, min_parallax_deg: float = 1.0, min_landmarks: int = 30, baseline: float = 1.0, hypotheses: int = 512,
                 refine_iterations: int = 4, seed: int = 0, ctx=None, pnp_sample: str = "dlt6"):
        self.pnp_sample = check_sample(pnp_sample, "pnp_sample")
        self.K = check_camera("K", K)
        self.threshold, self.baseline = check_scalars(threshold, baseline)
        self._cos2 = check_parallax(min_parallax_deg)
        self.min_parallax_deg = float(min_parallax_deg)
        self.min_landmarks = check_min_landmarks(min_landmarks)
        self.hypotheses, self.refine_iterations, self.seed = check_counts(hypotheses, refine_iterations, seed)
        check_ctx(ctx)
        self._ctx = ctx
        self._pnp = PnpRansac(self.K, self.hypotheses, self.threshold, self.refine_iterations, self.seed, ctx=ctx, sample=self.pnp_sample)
        self._filter = TwoViewRansac("auto", self.hypotheses, self.threshold, seed=self.seed, ctx=ctx)
        self._two_view = TwoViewPose(self.K, threshold=self.threshold, baseline=self.baseline, ctx=ctx)
        self.initialised, self.frame = False, 0
        self._anchored = False  # the bootstrap has its anchors
        self._n = None
        self._bound = {}
        self.pose = self.landmarks = self.owner = self.anchor_uv = self.anchor_pose = self.anchor_frame = self.pnp_status = self.anchor_status = None
        self.counters = self.valid = self.n_new = self.n_anchored = self.n_landmarks = self.n_dropped = self.lost = None

    # ---- the caller's side ------------------------------------------------------------------------------------------------------

    def reset(self) -> "TrackOdometry":
        """Forgets the map: the next call starts a bootstrap.  The next table may have another size."""
        self.initialised, self.frame, self._anchored = False, 0, False
        self._bound = {}
        if self.owner is not None:
            with OnStream(self._ctx, self.owner):
                self._empty_table()
            self._n = None
        return self

    def update(self, ids, points, image_size) -> "TrackOdometry":
        """The next frame of the track table (``image_size``: (H, W), for the bootstrap's filter).  Returns self."""
        from . import device as D

        rows, cols, _, _, _ = check_sizes(image_size, self.threshold, self.hypotheses, self.seed)
        complain((("ids", ids, _I64, (None,)), ("points", points, D._F32, (None, 2))))
        n = int(ids.shape[0])
        if not 1 <= n <= N.FTK_TRACK_TABLE_MAX_SLOTS:
            raise ValueError(f"ids must have 1 .. FTK_TRACK_TABLE_MAX_SLOTS = {N.FTK_TRACK_TABLE_MAX_SLOTS} slots (got {n})")
        if int(points.shape[0]) != n:
            raise ValueError(f"points must have one row per slot of ids, {n} (got {int(points.shape[0])})")
        index = getattr(self._ctx, "device_index", None)
        if points.device != ids.device or (index is not None and ids.device.index != index):
            raise ValueError(f"ids and points must be on one device, the context's (got {ids.device} and {points.device}"
                             + (")" if index is None else f", the context is on cuda:{index})"))
        if self._n is not None and (n != self._n or ids.device != self.owner.device):
            raise ValueError(f"the table so far has {self._n} slots on {self.owner.device} (got {n} on {ids.device}): call reset() before another table")
        with OnStream(self._ctx, ids) as on:
            if self.owner is None or self._n is None:
                self._allocate(on.torch, ids.device, n)
            self._bind(on, ids, points)
            if self.initialised:
                self._steady(on, points)
            elif not self._anchored:
                self._anchor_all(on)
            else:
                self._bootstrap(on, points, (rows, cols))
        self.frame += 1
        return self

    # ---- inside -----------------------------------------------------------------------------------------------------------------

    def _allocate(self, torch, device, n):
        if self.owner is None or int(self.owner.shape[0]) != n or self.owner.device != device:
            i32, f32 = dict(dtype=torch.int32, device=device), dict(dtype=torch.float32, device=device)
            self.owner = torch.empty(n, dtype=torch.int64, device=device)
            self.landmarks, self.anchor_uv, self.anchor_pose = torch.empty((n, 3), **f32), torch.empty((n, 2), **f32), torch.empty((n, 7), **f32)
            self.anchor_frame = torch.empty(n, **i32)
            self.pnp_status, self.anchor_status = torch.empty(n, dtype=torch.uint8, device=device), torch.empty(n, dtype=torch.uint8, device=device)
            self.counters, self.pose = torch.empty(N.FTK_LANDMARK_TABLE_COUNTERS, **i32), torch.empty(7, **f32)
            c = self.counters
            self.valid, self.n_new, self.n_anchored = c[N.FTK_LANDMARK_TABLE_VALID:][:1], c[N.FTK_LANDMARK_TABLE_N_NEW:][:1], c[N.FTK_LANDMARK_TABLE_N_ANCHORED:][:1]
            self.n_landmarks, self.n_dropped = c[N.FTK_LANDMARK_TABLE_N_LANDMARKS:][:1], c[N.FTK_LANDMARK_TABLE_N_DROPPED:][:1]
            self.lost = c[N.FTK_LANDMARK_TABLE_LOST:][:1]
            self._identity = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], **f32)
            self._one = torch.ones(1, **i32)
            self._empty_table()
        self._n = n

    def _empty_table(self):
        self.owner.fill_(-1)
        self.landmarks.zero_()
        self.anchor_uv.zero_()
        self.anchor_pose.zero_()
        self.anchor_frame.fill_(-1)
        self.pnp_status.zero_()
        self.anchor_status.zero_()
        self.counters.zero_()
        self.pose.copy_(self._identity)

    def _bind(self, on, ids, points):
        """The two entries' arguments, marshalled once per (ids, points) and kept: the table's own tensors are fixed."""
        if self._bound.get("ids") is ids and self._bound.get("points") is points and self._bound.get("ctx") is on.ctx:
            return
        begin = list(landmark_begin_args(on.ctx, ids, self.owner, self.landmarks, self.anchor_frame, self.pnp_status, self.anchor_status, self.counters, on.stream))
        end = list(landmark_end_args(on.ctx, ids, points, self.pnp_status, self._identity, self._one, None, 0, N.FTK_LANDMARK_TABLE_STEADY, self.K, self.threshold,
                                     self._cos2, self.landmarks, self.anchor_uv, self.anchor_pose, self.anchor_frame, self.counters, self.pose, on.stream))
        self._bound = dict(ids=ids, points=points, ctx=on.ctx, begin=begin, end=end, status=end[END_STATUS_ARG])

    def _begin(self, on):
        args = self._bound["begin"]
        args[STREAM_ARG] = C.c_void_p(on.stream.cuda_stream)  # this call's stream: torch's current one when the context has none (a capture's, say)
        call("ftk_landmark_table_begin_device", args, on.ctx)

    def _end(self, on, mode, pose_in, valid_in, model_in=None):
        """``pose_in`` / ``valid_in`` / ``model_in``: float32 [7] / int32 [1] / int32 [1] tensors that this package's classes made."""
        from . import device as D

        dev = D._call_device(on.ctx, pose_in)
        D._check("pose_in", pose_in, D._F32, (7,), dev)
        D._check("valid_in", valid_in, D._I32, (1,), dev)
        if model_in is not None:
            D._check("model_in", model_in, D._I32, (1,), dev)
        args = self._bound["end"]
        args[STREAM_ARG] = C.c_void_p(on.stream.cuda_stream)
        args[END_STATUS_ARG] = self._bound["status"] if mode == N.FTK_LANDMARK_TABLE_STEADY else None
        args[END_POSE_ARG], args[END_VALID_ARG], args[END_MODEL_ARG] = pointer(pose_in), pointer(valid_in), pointer(model_in)
        args[END_FRAME_ARG], args[END_MODE_ARG] = self.frame, mode
        call("ftk_landmark_table_end_device", args, on.ctx)

    def _frame_seed(self):
        return (self.seed + self.frame) & 0xFFFFFFFF

    def _anchor_all(self, on):
        """Every live slot anchored at this frame with the identity pose: the end kernel in steady mode on a table without landmarks."""
        self._begin(on)
        self._end(on, N.FTK_LANDMARK_TABLE_STEADY, self._identity, self._one)
        self._anchored = True

    def _steady(self, on, points):
        self._begin(on)
        fit = self._pnp.solve(self.landmarks, points, self.pnp_status, seed=self._frame_seed())
        self._end(on, N.FTK_LANDMARK_TABLE_STEADY, fit.pose, fit.valid)

    def _bootstrap(self, on, points, image_size):
        self._begin(on)
        fit = self._filter.filter(self.anchor_uv, points, self.anchor_status, image_size, seed=self._frame_seed())
        two = self._two_view.solve(self.anchor_uv, points, self.anchor_status)
        self._end(on, N.FTK_LANDMARK_TABLE_BOOTSTRAP, two.pose, two.valid, fit.model)
        valid, n_new, n_anchored = self.counters[:3].tolist()  # VALID, N_NEW, N_ANCHORED: the one host read, one copy
        if valid == 1 and n_new >= self.min_landmarks:
            self.initialised = True
            return
        self.landmarks.zero_()
        self.n_landmarks.zero_()
        self.n_new.zero_()  # (the attempt's landmarks were discarded)
        self.pose.copy_(self._identity)
        if n_anchored < self.min_landmarks:  # too few of the anchors' tracks are left: the pair starts again from this frame
            self.anchor_frame.fill_(-1)
            self._anchor_all(on)
