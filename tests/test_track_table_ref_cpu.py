"""The numpy restatement of masked Harris selection, retire and fill (tests/track_table_ref.py) held to the oracle where
the oracle speaks (no occupied point), to the contract's invariants elsewhere, and shown to notice each of five plausible mistakes."""
import os

import numpy as np
import pytest

from feature_tracker_amd import synth
from tests import klt_video_cases as K
from tests import oracle_lib
from tests import track_table_ref as R

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "optical_flow")
SIZES = [(23, 23), (24, 40), (64, 48), (333, 251)]
DISTANCES = [1, 2, 9, 25]


def _scene(width, height):
    return np.ascontiguousarray(synth.make_image_pair(max(width, 32), max(height, 32), (0.0, 0.0))[0][:height, :width])


@pytest.mark.parametrize("distance", DISTANCES)
@pytest.mark.parametrize("width,height", SIZES + [(None, None)])
def test_without_occupied_points_it_is_the_oracle(width, height, distance):
    if width is None:
        from PIL import Image
        image = np.array(Image.open(os.path.join(DATA, "ref_image.png")))
    else:
        image = _scene(width, height)
    want = oracle_lib.harris_detect(image, image.size, distance, 40.0)
    got = R.masked_survivors(image, distance, 40.0)
    assert np.array_equal(got, want)
    uv, n = R.detect(image, 7, distance, 40.0)
    assert n == min(7, len(want)) and np.array_equal(uv[:n], want[:n]) and not uv[n:].any()
    assert len(want) <= max(R.survivor_bound(image.shape[0], image.shape[1], distance), 0)


def _chebyshev(a, b):
    return np.abs(a[:, None, :] - b[None, :, :]).max(axis=2)


@pytest.mark.parametrize("distance", [2, 9, 25])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_invariants_on_random_occupied_sets(distance, seed):
    image = _scene(160, 120)
    rs = np.random.RandomState(seed)
    occupied = np.stack([rs.uniform(-3, 163, 40), rs.uniform(-3, 123, 40)], axis=1).astype(np.float32)
    mask = (rs.uniform(size=40) < 0.8).astype(np.uint8)
    got = R.masked_survivors(image, distance, 40.0, occupied, mask)
    assert len(got) > 0 and len(got) <= R.survivor_bound(120, 160, distance)
    assert (_chebyshev(got, got) + np.eye(len(got)) * 1e9).min() >= distance
    stamped = np.array(R.stamps(occupied, mask, 120, 160), np.float32)
    assert _chebyshev(got, stamped).min() >= distance
    # every corner the unmasked detector finds away from the stamps' doubled reach is still found: blocking is local
    free = R.masked_survivors(image, distance, 40.0)
    far = free[_chebyshev(free, stamped).min(axis=1) >= 2 * distance]
    assert {tuple(p) for p in far} <= {tuple(p) for p in got}


@pytest.mark.parametrize("name", ["basic_fast", "more_slots_than_corners", "more_slots_than_a_retire_block", "large_shift", "forward_backward", "reset_mid_sequence"])
def test_table_invariants_over_a_sequence(name):
    states, _ = K.reference_run(name)
    seen, top = set(), -1
    for k, s in enumerate(states):
        live = s["ids"] >= 0
        assert int(s["n_live"][0]) == int(live.sum())
        assert (s["status"][live] <= R.TRACKED).all() and (s["status"][~live] > R.TRACKED).all()  # empty slots are never tracked
        ids = s["ids"][live]
        assert len(set(ids.tolist())) == len(ids) and (ids < s["next_id"][0]).all()
        fresh = s["ids"][live & (s["age"] == 0)]
        assert (fresh > top).all() and not (set(fresh.tolist()) & seen)  # identities are never reused
        assert (np.diff(fresh) > 0).all()  # free slots fill in ascending order, ids increase with rank: fresh ids ascend with the slot index
        seen |= set(ids.tolist())
        top = max(top, int(s["next_id"][0]) - 1)
        pts = s["points"][live]
        assert (_chebyshev(pts[s["age"][live] == 0], pts[s["age"][live] == 0]) + np.eye(int((s["age"][live] == 0).sum())) * 1e9).min(initial=1e9) >= K.MIN_DISTANCE


def _sequence_with(mutant):
    """A short table history under one mutant: two detections around a hand-made retirement."""
    image = _scene(160, 120)
    table = R.Table(48)
    table.detect_and_fill(image, 9, 40.0, mutant)
    tracked = table.points + np.float32(0.4)  # 0.4: floor(x + 0.5) and trunc(x) still agree; the half-pixel case is below
    status = np.full(48, R.TRACKED, np.uint8)
    status[[30, 5, 17]] = R.OUTSIDE
    table.ids[[40, 41]] = -1  # (as if retired a frame earlier and never refilled)
    table.status[[40, 41]] = R.OUTSIDE
    table.retire(tracked, status, mutant=mutant)
    table.points[table.ids >= 0] += np.float32(0.2)  # live points now sit at x.6: truncation stamps one pixel to the left and up
    table.detect_and_fill(image, 9, 40.0, mutant)
    few = R.Table(200)
    few.detect_and_fill(image, 9, 40.0, mutant)  # more free slots than corners
    return table.tensors(), few.tensors()


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_each_mutant_is_caught(mutant):
    good, bad = _sequence_with(None), _sequence_with(mutant)
    same = all(np.array_equal(g[t], b[t]) for g, b in zip(good, bad) for t in g)
    assert not same, f"the mutant {mutant} changes nothing these cases see"


def test_forward_backward_error_is_one_fused_rounding():
    assert R.fb_error2((1.5, 2.25), (1.0, 2.0)) == np.float32(0.3125)
    # dy * dy + fl(dx * dx) rounded once: differs from the twice-rounded sum here
    dx, dy = np.float32(1.0000001), np.float32(0.00034526698)
    fused = R.fb_error2((dx, dy), (0.0, 0.0))
    exact = float(dy) * float(dy) + float(np.float32(dx * dx))
    assert abs(float(fused) - exact) <= abs(float(np.float32(np.float32(dy * dy) + np.float32(dx * dx))) - exact)
