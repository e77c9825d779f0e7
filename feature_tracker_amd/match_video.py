"""``MatchVideoTracker``: learned features over a frame sequence, on a landmark table that lives on the device.

``SuperPoint`` -> ``KeypointDecoder`` -> ``LightGlue`` / ``MatchAssignment`` -> ``TwoViewRansac`` runs from two images to filtered index
pairs; a caller who wants TRACKS (stable ids, ages, where each landmark was last seen) had to run the detector twice per pair, read
``match_index`` back and keep the ids in Python.  Here that loop is one call per frame: the matcher is asked about the table (the last
seen position and descriptor of every live track), not about the previous frame's detections, so a landmark that was hidden for up to
``max_lost`` frames is found again under its identity.  No copy to the host, no count read back, no synchronisation.
"""
from __future__ import annotations

import math

from . import _native as N
from ._device_epipolar import check_sizes as check_ransac_sizes
from ._device_match_table import check_max_lost, match_table_query_args, match_table_update_args
from ._torch_call import OnStream, PerKey, call, check_ctx, complain, words
from .tracker import LARGE_RESIDUAL, OUTSIDE


class MatchVideoTracker:
    """``tracker.update(uv, descriptors, count, image_size)`` or ``tracker.track(image)`` once per frame; afterwards the table is in the
    attributes, valid until the next call:

    =========== =================== ==========================================
    ids         int64 [N]           -1 = empty
    points      float32 [N, 2]      where the landmark was last seen, (u, v)
    prev_points float32 [N, 2]      where it was seen before that
    descriptors float32 [N, D]      its descriptor when last seen (replaced, not averaged)
    status      uint8 [N]           TRACKED: matched in this frame; LARGE_RESIDUAL: not; NOT_TRACKED: admitted in this frame
    age         int32 [N]           frames matched since admission
    lost        int32 [N]           frames since it was last matched
    n_live      int32 [1]           live slots
    next_id     int64 [1]           the next identity to hand out
    cur_slot    int32 [K]           per current row: the slot it now belongs to, or -1
    =========== =================== ==========================================

    Slots never move.  Per frame: the live slots become the matcher's reference set (``ftk_match_table_query_device``), the matcher runs
    on it against the current keypoints, the optional geometric filter rewrites the match status, and
    ``ftk_match_table_update_device`` carries the result into the table: a matched slot moves on, an unmatched one ages and retires once
    ``lost > max_lost`` (``max_lost=0`` is pairwise matching: a track dies on its first miss), and the current keypoints no slot named
    fill the empty slots, strongest first, under new ids.  A keypoint whose match the filter rejected is not admitted.  The first frame
    after construction or ``reset()`` runs no matcher: everything is admitted.

    ``matcher``: a ``LightGlue`` (called with keypoints, ``image_size`` and counts) or a ``MatchAssignment`` (descriptors only);
    ``adaptive=True`` uses ``LightGlue.match_adaptive``.  ``detector=(superpoint, decoder)`` enables ``track(image)``.  ``geometric``: a
    ``TwoViewRansac`` or an ``EpipolarRansac``; frame f (counted from construction or ``reset()``) uses the seed ``geometric_seed + f``.

    Limits: one camera, float32, ``max_tracks`` and current rows in 1 .. 4 096 (the matchers' row limit), no CPU fallback, no C++ class.
    The two table entries are capturable; the tracker is not promised to be (it has state)."""

    def __init__(self, matcher, max_tracks: int, max_lost: int = 0, min_score: float = -1.0e30, adaptive: bool = False, detector=None, geometric=None,
                 geometric_seed: int = 0, ctx=None):
        from .epipolar import EpipolarRansac
        from .keypoint_decoder import KeypointDecoder
        from .match_assignment import MatchAssignment
        from .superpoint import SuperPoint
        from .transformer import LightGlue
        from .two_view import TwoViewRansac

        if isinstance(matcher, LightGlue):
            self._kind = "lightglue"
            self.dim = matcher.dim if matcher.input_proj is None else int(matcher.input_proj[0].shape[1])
        elif isinstance(matcher, MatchAssignment):
            self._kind = "assignment"
            self.dim = matcher.dim
        else:
            raise ValueError(f"matcher must be a LightGlue or a MatchAssignment (got {type(matcher).__name__})")
        if isinstance(max_tracks, bool) or not isinstance(max_tracks, int) or not 1 <= max_tracks <= N.FTK_MATCH_TABLE_MAX_SLOTS:
            raise ValueError(f"max_tracks must be an integer in 1 .. FTK_MATCH_TABLE_MAX_SLOTS = {N.FTK_MATCH_TABLE_MAX_SLOTS} (got {max_tracks!r})")
        self.max_lost = check_max_lost(max_lost)
        if isinstance(min_score, bool) or not isinstance(min_score, (int, float)) or math.isnan(min_score):
            raise ValueError(f"min_score must be a number (got {min_score!r})")
        if adaptive:
            if self._kind != "lightglue":
                raise ValueError("adaptive=True needs a LightGlue: a MatchAssignment has no layers to stop early")
            if matcher._adaptive is None:
                raise ValueError("adaptive=True needs LightGlue.from_state_dict(..., depth_confidence=..., width_confidence=...) with one of them > 0")
        if detector is not None:
            if not isinstance(detector, (tuple, list)) or len(detector) != 2 or not isinstance(detector[0], SuperPoint) or not isinstance(detector[1], KeypointDecoder):
                raise ValueError(f"detector must be (SuperPoint, KeypointDecoder) (got {detector!r})")
            if detector[0].descriptor_channels != self.dim:
                raise ValueError(f"the detector's descriptors have {detector[0].descriptor_channels} channels, the matcher takes {self.dim}")
            if detector[1].max_keypoints > N.FTK_MATCH_TABLE_MAX_SLOTS:
                raise ValueError(f"the decoder's max_keypoints {detector[1].max_keypoints} exceeds FTK_MATCH_TABLE_MAX_SLOTS = {N.FTK_MATCH_TABLE_MAX_SLOTS}")
        if geometric is not None and not isinstance(geometric, (TwoViewRansac, EpipolarRansac)):
            raise ValueError(f"geometric must be a TwoViewRansac or an EpipolarRansac (got {type(geometric).__name__})")
        if isinstance(geometric_seed, bool) or not isinstance(geometric_seed, int) or not 0 <= geometric_seed <= 0xFFFFFFFF:
            raise ValueError(f"geometric_seed must be a uint32 (got {geometric_seed!r})")
        check_ctx(ctx)
        self.matcher, self.max_tracks, self.min_score, self.adaptive = matcher, max_tracks, float(min_score), bool(adaptive)
        self.detector, self.geometric, self.geometric_seed = detector, geometric, geometric_seed
        self._ctx = ctx
        self._frames = 0
        self._device = None
        self._per_rows = PerKey()  # K -> the buffers of a frame of that many current rows
        self.ids = self.points = self.prev_points = self.descriptors = self.status = self.age = self.lost = self.n_live = self.next_id = None
        self.cur_slot = None

    # ---- the caller's side ------------------------------------------------------------------------------------------------------

    def reset(self) -> "MatchVideoTracker":
        """Empties the table; identities go on from ``next_id``."""
        self._frames = 0
        if self.ids is not None:
            with OnStream(self._ctx, self.ids):
                self._empty_table()
        return self

    def live(self):
        """(ids, points, prev_points, age, lost) of the live slots, by boolean indexing: the one place that synchronises."""
        if self.ids is None:
            raise RuntimeError("MatchVideoTracker.live() before the first update()")
        keep = self.ids >= 0
        return self.ids[keep], self.points[keep], self.prev_points[keep], self.age[keep], self.lost[keep]

    def track(self, image) -> "MatchVideoTracker":
        """The next frame as an image: ``update`` on ``superpoint.detect(image, decoder)``.  ``image`` as ``SuperPoint`` takes it."""
        if self.detector is None:
            raise ValueError("track(image) needs detector=(superpoint, decoder) at construction: update(uv, descriptors, ...) takes keypoints")
        superpoint, decoder = self.detector
        H, W = superpoint._check_image(image)
        found = superpoint.detect(image, decoder)
        return self.update(found.uv, found.descriptors, found.count, image_size=(W, H))

    def update(self, uv, descriptors, count=None, image_size=None) -> "MatchVideoTracker":
        """The next frame as keypoints: ``uv`` float32 CUDA [K, 2], ``descriptors`` [K, D], strongest first as ``KeypointDecoder`` orders
        them; ``count``: int32 [1] device tensor or None (all K rows); ``image_size``: (W, H), required with a ``LightGlue`` or a
        geometric filter.  Returns self; everything is enqueued."""
        k, size = self._validate(uv, descriptors, count, image_size)
        n = self.max_tracks
        from . import device as D

        with OnStream(self._ctx, uv) as on:
            torch, ctx, stream, device = on.torch, on.ctx, on.stream, uv.device
            if self.ids is None:
                self._allocate(torch, device)
            elif device != self._device:
                raise ValueError(f"uv is on {device}, the table on {self._device}")
            call("ftk_match_table_query_device",
                 match_table_query_args(ctx, self.ids, self.points, self.descriptors, self._q_uv, self._q_desc, self._q_slot, self._q_count, stream), ctx)
            per = self._per_rows.of(k, lambda: self._allocate_rows(torch, device, k))
            match_index, match_status = self._no_index, self._no_status
            if self._frames > 0:
                match_index, match_status = self._match(uv, descriptors, count, size)
                if self.geometric is not None:
                    cur = uv
                    if k < n:  # the pixel fill addresses row t of the current set for every query row t: give it n rows
                        cur = per["cur_pad"]
                        cur[:k].copy_(uv)
                    D.nn_fill_pixels_device(ctx, match_index, cur, per["matched"], stream)
                    self.geometric.filter(self._q_uv, per["matched"][:n], match_status, (size[1], size[0]), seed=(self.geometric_seed + self._frames) & 0xFFFFFFFF)
            args = match_table_update_args(ctx, self.ids, self.points, self.prev_points, self.descriptors, self.status, self.age, self.lost, self.n_live,
                                           self.next_id, self._q_slot, self._q_count, match_index, match_status, uv, descriptors, count, self.max_lost,
                                           per["workspace"], per["cur_slot"], stream)
            call("ftk_match_table_update_device", args, ctx)
            self.cur_slot = per["cur_slot"]
        self._frames += 1
        return self

    # ---- inside -----------------------------------------------------------------------------------------------------------------

    def _validate(self, uv, descriptors, count, image_size):
        """(K, (W, H) or None), or the ValueError: before anything touches a device."""
        from . import device as D
        from .transformer import _check_size

        tensors = [("uv", uv, D._F32, (None, 2)), ("descriptors", descriptors, D._F32, (None, self.dim))]
        complain(tensors, cuda=False)
        k = int(uv.shape[0])
        if not 1 <= k <= N.FTK_MATCH_TABLE_MAX_SLOTS:
            raise ValueError(f"uv must have 1 .. FTK_MATCH_TABLE_MAX_SLOTS = {N.FTK_MATCH_TABLE_MAX_SLOTS} rows (got {k})")
        tensors[1] = ("descriptors", descriptors, D._F32, (k, self.dim))
        if count is not None:
            tensors.append(("count", count, D._I32, (1,)))
        if image_size is None:
            if self._kind == "lightglue":
                raise ValueError("image_size=(W, H) is required with a LightGlue: its positional encoding normalises the keypoints by it")
            if self.geometric is not None:
                raise ValueError("image_size=(W, H) is required with a geometric filter: it normalises the coordinates by it")
        else:
            _check_size("image_size", image_size)
            if self.geometric is not None:
                check_ransac_sizes((image_size[1], image_size[0]), self.geometric.threshold, self.geometric.hypotheses, 0)
        complain(tensors)
        return k, image_size

    def _match(self, uv, descriptors, count, size):
        """The matcher on the query rows against the current set: (match_index int32 [N], status uint8 [N]) on the device."""
        m = self.matcher
        if self._kind == "assignment":
            _, index, status = m.match(self._q_desc, descriptors, self._q_count, count, min_score=self.min_score)
        elif self.adaptive:
            found = m.match_adaptive(self._q_uv, uv, self._q_desc, descriptors, size, size, self._q_count, count, min_score=self.min_score)
            index, status = found.match_index, found.status
        else:
            _, index, status = m.match(self._q_uv, uv, self._q_desc, descriptors, size, size, self._q_count, count, min_score=self.min_score)
        return index, status

    def _allocate(self, torch, device):
        n, d = self.max_tracks, self.dim
        self._device = device
        self.ids = torch.empty(n, dtype=torch.int64, device=device)
        self.points = torch.empty((n, 2), dtype=torch.float32, device=device)
        self.prev_points = torch.empty((n, 2), dtype=torch.float32, device=device)
        self.descriptors = torch.empty((n, d), dtype=torch.float32, device=device)
        self.status = torch.empty(n, dtype=torch.uint8, device=device)
        self.age = torch.empty(n, dtype=torch.int32, device=device)
        self.lost = torch.empty(n, dtype=torch.int32, device=device)
        self.n_live = torch.empty(1, dtype=torch.int32, device=device)
        self.next_id = torch.zeros(1, dtype=torch.int64, device=device)
        self._q_uv = torch.empty((n, 2), dtype=torch.float32, device=device)
        self._q_desc = torch.empty((n, d), dtype=torch.float32, device=device)
        self._q_slot = torch.empty(n, dtype=torch.int32, device=device)
        self._q_count = torch.empty(1, dtype=torch.int32, device=device)
        # what the first frame's update reads instead of a matcher's results: no row names anything (and nq is 0)
        self._no_index = torch.full((n,), -1, dtype=torch.int32, device=device)
        self._no_status = torch.full((n,), LARGE_RESIDUAL, dtype=torch.uint8, device=device)
        self._empty_table()

    def _allocate_rows(self, torch, device, k):
        n = self.max_tracks
        per = dict(workspace=words(torch, N.match_table_workspace_bytes(n, k, self.dim), device),
                   cur_slot=torch.empty(k, dtype=torch.int32, device=device))
        if self.geometric is not None:
            per["matched"] = torch.zeros((max(n, k), 2), dtype=torch.float32, device=device)
            if k < n:
                per["cur_pad"] = torch.zeros((n, 2), dtype=torch.float32, device=device)
        return per

    def _empty_table(self):
        self.ids.fill_(-1)
        self.points.zero_()
        self.prev_points.zero_()
        self.descriptors.zero_()
        self.status.fill_(OUTSIDE)
        self.age.zero_()
        self.lost.zero_()
        self.n_live.zero_()
