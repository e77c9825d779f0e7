"""KltVideoTracker on the device against the restatement composed with the oracle's trackers (tests/track_table_ref.py,
tests/klt_video_cases.py): after every frame all seven tensors of the table are equal bit for bit."""
import numpy as np
import pytest

from tests import klt_video_cases as K

pytestmark = pytest.mark.gpu

TENSORS = ("ids", "points", "prev_points", "status", "age", "n_live", "next_id")


def _tracker(ftk, name):
    model, method, slots, _, _, fb, _ = K.CASES[name]
    flow = {"basic": ftk.OpticalFlowBasicKlt, "affine": ftk.OpticalFlowAffineKlt, "lssd": ftk.OpticalFlowLssdKlt}[model]()
    flow.options().kMethod = method
    flow.options().kMaxTrackPointsNumber = max(slots, 500)
    return ftk.KltVideoTracker(flow, slots, levels=K.LEVELS, min_distance=K.MIN_DISTANCE, min_response=K.MIN_RESPONSE, forward_backward=fb)


def _run(ftk, name, as_tensor=True):
    """The device tracker over the case's frames: per frame a host copy of the seven tensors."""
    import torch
    _, _, _, motion, rotation, _, reset_before = K.CASES[name]
    tracker, states = _tracker(ftk, name), []
    for k, image in enumerate(K.frames(motion, rotation)):
        if reset_before == k:
            tracker.reset()
        tracker.track(torch.from_numpy(image).cuda() if as_tensor else image)
        states.append({t: getattr(tracker, t).cpu().numpy() for t in TENSORS})
    return tracker, states


def _same(got, want, what):
    for t in TENSORS:
        g, w = got[t], want[t]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, t, g.dtype, g.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, f"{what}: {t} differs in {bad.size} rows, first {bad[:5]}: got {got[t][bad[:5]]}, want {want[t][bad[:5]]}"


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_every_frame_equals_the_restatement(ftk, oracle, name):
    want, (fb_retired, fb_passed) = K.reference_run(name)
    tracker, got = _run(ftk, name)
    for k, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"{name}, frame {k}")
    slots, fb, reset_before = K.CASES[name][2], K.CASES[name][5], K.CASES[name][6]
    last = want[-1]
    if name == "more_slots_than_corners":
        assert (last["ids"] < 0).sum() > 0 and (last["status"][last["ids"] < 0] > 1).all()  # empty slots persist, and are skipped
    if name == "large_shift":
        changed = np.flatnonzero(want[2]["ids"] != want[1]["ids"])  # slots died at the border and were refilled with fresh ids
        assert last["next_id"][0] > slots and changed.size > 0 and (want[2]["ids"][changed] >= want[1]["next_id"][0]).all()
    if fb is not None:
        assert fb_retired >= 1 and fb_passed >= 1
    if reset_before is not None:
        before, after = want[reset_before - 1], want[reset_before]
        assert after["ids"][after["ids"] >= 0].min() == before["next_id"][0] and (after["age"] == 0).all()  # ids go on
    ids, points, prev_points, age = tracker.live()
    keep = last["ids"] >= 0
    assert np.array_equal(ids.cpu().numpy(), last["ids"][keep]) and np.array_equal(points.cpu().numpy(), last["points"][keep])
    assert np.array_equal(prev_points.cpu().numpy(), last["prev_points"][keep]) and np.array_equal(age.cpu().numpy(), last["age"][keep])


def test_first_frame_is_detect_good_features(ftk):
    _, states = _run(ftk, "basic_fast")
    image = K.frames(*K.CASES["basic_fast"][3:5])[0]
    det = ftk.FeaturePointHarrisDetector()
    det.options().kMinFeatureDistance, det.options().kMinValidResponse = K.MIN_DISTANCE, K.MIN_RESPONSE
    ok, uv = det.DetectGoodFeatures(image, 64)
    n = int(states[0]["n_live"][0])
    assert ok and n == len(uv) and np.array_equal(states[0]["points"][:n], uv) and np.array_equal(states[0]["ids"][:n], np.arange(n))


def test_two_runs_give_identical_tables(ftk):
    """The survivors reach the device's list in the order of an atomicAdd; the tables must not show it.  A numpy frame is uploaded, a
    tensor read in place: the same tables either way."""
    _, first = _run(ftk, "large_shift")
    _, second = _run(ftk, "large_shift", as_tensor=False)
    for k, (a, b) in enumerate(zip(first, second)):
        _same(a, b, f"run 1 against run 2, frame {k}")


def test_shape_change_needs_reset(ftk):
    import torch
    tracker = _tracker(ftk, "one_slot")
    tracker.track(torch.zeros(40, 48, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match=r"call reset\(\)"):
        tracker.track(torch.zeros(48, 40, dtype=torch.uint8, device="cuda"))
    tracker.reset().track(torch.zeros(48, 40, dtype=torch.uint8, device="cuda"))
    assert int(tracker.n_live.item()) == 0 and int(tracker.next_id.item()) == 0  # a flat image has no corner
