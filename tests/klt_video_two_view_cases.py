"""Shared by tests/test_klt_video_two_view_gpu.py and tests/test_two_view_args_cpu.py: KltVideoTracker with ``epipolar_model`` restated —
tests/track_table_ref.py and the oracle's trackers over the sequences of tests/klt_video_cases.py and tests/klt_video_epipolar_cases.py
(imported, not edited), with tests/two_view_ref.py between the forward call and the backward call — and "planar_patch", a sequence of this
file's own: ONE plane (the whole image moves by BACKGROUND a frame, what a camera sees that translates parallel to a wall) and a patch
that moves another way, 7.1 pixels a frame from where the plane's motion would put it, against a threshold of 1.  One plane leaves a
three-parameter family of fundamental matrices, so the fundamental route is permissive here; the homography is not."""
import functools

import numpy as np

from feature_tracker_amd import synth
from tests import klt_video_cases as K
from tests import klt_video_epipolar_cases as V
from tests import oracle_lib
from tests import track_table_ref as R
from tests import two_view_ref as T

THRESHOLD, SEED, PREFER = V.THRESHOLD, V.SEED, 750
NAMES = ("basic_fast", "forward_backward")

WIDTH, HEIGHT, SLOTS, HYPOTHESES = V.PATCH_WIDTH, V.PATCH_HEIGHT, V.PATCH_SLOTS, V.PATCH_HYPOTHESES
BACKGROUND, PATCH_MOTION = (3.0, 1.0), (-2.0, 6.0)  # (u, v) pixels a frame; the difference is (-5, 5): 7.1 pixels


def _moved(shift, k):
    if k == 0:
        return synth.make_image_pair(WIDTH, HEIGHT, (0.0, 0.0))[0]
    return synth.make_image_pair(WIDTH, HEIGHT, (k * shift[0], k * shift[1]))[1]


@functools.lru_cache(maxsize=None)
def frames(name):
    if name != "planar_patch":
        return V.frames(name)
    r0, r1, c0, c1 = V.PATCH
    out = []
    for k in range(K.FRAMES):
        frame = _moved(BACKGROUND, k).copy()
        frame[r0:r1, c0:c1] = _moved(PATCH_MOTION, k)[r0:r1, c0:c1]
        out.append(np.ascontiguousarray(frame))
    return tuple(out)


def config(name):
    """(model, method, slots, forward-backward threshold, frame before which reset() is called, hypotheses, (H, W))"""
    if name == "planar_patch":
        return "basic", "fast", SLOTS, None, None, HYPOTHESES, (HEIGHT, WIDTH)
    return V.config(name)


@functools.lru_cache(maxsize=None)
def reference_run(name, epipolar_model):
    """Per frame a copy of the seven tensors, and per tracked frame (forward status before the filter, after it, the restatement's result,
    the points the frame started from)."""
    model, method, slots, fb, reset_before, hypotheses, size = config(name)
    table = R.Table(slots)
    states, fits, prev, tracked_frames = [], [], None, 0
    for k, image in enumerate(frames(name)):
        levels = oracle_lib.create_pyramid(image, K.LEVELS)
        if reset_before == k:
            table.empty()
            tracked_frames = 0
        if tracked_frames == 0:
            table.detect_and_fill(image, K.MIN_DISTANCE, K.MIN_RESPONSE)
        else:
            kw = dict(prior=None, consider_luminance=False, max_points=max(table.n, 1), method=method, half=6)
            _, uv, st, _ = oracle_lib.klt_track_pyramid(model, prev, levels, table.points, table.points.copy(), table.status.copy(), **kw)
            fit = T.ransac(table.points, uv, st, size, THRESHOLD, hypotheses, SEED + tracked_frames, epipolar_model, PREFER)  # the seed of frame f
            fits.append((st.copy(), fit.status.copy(), fit, table.points.copy()))
            back_uv = back_st = None
            if fb is not None:  # the backward call starts from the filtered statuses: a rejected slot is passed through
                _, back_uv, back_st, _ = oracle_lib.klt_track_pyramid(model, levels, prev, uv, uv.copy(), fit.status.copy(), **kw)
            table.retire(uv, fit.status, back_uv, back_st, fb)
            table.detect_and_fill(image, K.MIN_DISTANCE, K.MIN_RESPONSE)
        prev = levels
        tracked_frames += 1
        states.append({k_: v.copy() for k_, v in table.tensors().items()})
    return states, fits


def verdicts(fits):
    """Per tracked frame V.patch_verdict: (tracked ON the patch, rejected of them, tracked OFF it, rejected of them)."""
    return [V.patch_verdict(before, after, points) for before, after, _, points in fits]
