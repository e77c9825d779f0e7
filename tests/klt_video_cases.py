"""Shared by tests/test_klt_video_gpu.py and tests/test_track_table_ref_cpu.py: the frame sequences, the tracker configurations and the
restatement's run over a sequence (tests/track_table_ref.py composed with the oracle's trackers)."""
import functools

import numpy as np

from feature_tracker_amd import synth
from tests import oracle_lib
from tests import track_table_ref as R

WIDTH, HEIGHT, LEVELS, FRAMES = 160, 120, 3, 5
MIN_DISTANCE, MIN_RESPONSE = 9, 40.0

# name -> (model, method, slots, motion per frame, rotation per frame in degrees, forward-backward threshold, frame before which reset() is called)
CASES = {
    "basic_fast": ("basic", "fast", 64, (3.3, -2.1), 0.0, None, None),
    "affine_inverse": ("affine", "inverse", 64, (3.3, -2.1), 0.5, None, None),
    "lssd_direct": ("lssd", "direct", 64, (3.3, -2.1), 0.5, None, None),
    "one_slot": ("basic", "fast", 1, (3.3, -2.1), 0.0, None, None),
    "more_slots_than_corners": ("basic", "fast", 512, (3.3, -2.1), 0.0, None, None),
    "more_slots_than_a_retire_block": ("basic", "fast", 1500, (3.3, -2.1), 0.0, None, None),
    "large_shift": ("basic", "fast", 64, (11.7, -8.4), 0.0, None, None),
    "forward_backward": ("basic", "fast", 64, (14.3, -10.2), 3.0, 1.0, None),
    "reset_mid_sequence": ("basic", "fast", 64, (3.3, -2.1), 0.0, None, 3),
}


@functools.lru_cache(maxsize=None)
def frames(motion, rotation):
    """FRAMES images of one scene: frame k is the scene moved by k * motion and turned by k * rotation degrees."""
    out = [synth.make_image_pair(WIDTH, HEIGHT, (0.0, 0.0))[0]]
    for k in range(1, FRAMES):
        out.append(synth.make_image_pair(WIDTH, HEIGHT, (k * motion[0], k * motion[1]), rotation_deg=k * rotation)[1])
    return tuple(np.ascontiguousarray(f) for f in out)


@functools.lru_cache(maxsize=None)
def reference_run(name):
    """The restatement over the case's sequence: per frame a copy of the seven tensors, plus (slots the forward-backward check retired,
    slots that passed it) over the whole run."""
    model, method, slots, motion, rotation, fb, reset_before = CASES[name]
    table = R.Table(slots)
    seq, states, prev, tracked_frames = frames(motion, rotation), [], None, 0
    fb_retired = fb_passed = 0
    for k, image in enumerate(seq):
        levels = oracle_lib.create_pyramid(image, LEVELS)
        if reset_before == k:
            table.empty()
            tracked_frames = 0
        if tracked_frames == 0:
            table.detect_and_fill(image, MIN_DISTANCE, MIN_RESPONSE)
        else:
            held = table.ids >= 0
            uv, st, back_uv, back_st = R.track_frame(table, model, prev, levels, image, MIN_DISTANCE, MIN_RESPONSE, forward_backward=fb, method=method, half=6)
            if fb is not None:
                forward_ok = held & (st == R.TRACKED)
                fb_passed += int((forward_ok & (table.status == R.TRACKED) & (table.age > 0)).sum())
                fb_retired += int((forward_ok & (table.status == R.LARGE_RESIDUAL)).sum())
        prev = levels
        tracked_frames += 1
        states.append({k_: v.copy() for k_, v in table.tensors().items()})
    return states, (fb_retired, fb_passed)
