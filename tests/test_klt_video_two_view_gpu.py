"""KltVideoTracker with ``epipolar_model`` on the device against its restatement (tests/klt_video_two_view_cases.py: the track table's and
the two-view restatements composed with the oracle's trackers): after every frame all seven tensors of the table are equal
bit for bit, for "homography" and "auto", with and without the forward-backward check; the default "fundamental" is the tracker without
the argument; on one plane with a patch that moves another way "auto" retires the patch's tracks where "fundamental" does not; on the
depth layers of "moving_patch" "auto" is the fundamental route."""
import numpy as np
import pytest

from tests import epipolar_ref as E
from tests import klt_video_cases as K
from tests import klt_video_epipolar_cases as V
from tests import klt_video_two_view_cases as W
from tests.test_klt_video_gpu import TENSORS, _same

pytestmark = pytest.mark.gpu


def _run(ftk, name, epipolar_model=None):
    """The device tracker over the case's frames: per frame a host copy of the seven tensors, and per tracked frame the fit it holds, its
    own forward statuses after the filter and the points the frame started from.  None: the tracker built without the argument."""
    import torch
    model, method, slots, fb, reset_before, hypotheses, _ = W.config(name)
    flow = {"basic": ftk.OpticalFlowBasicKlt, "affine": ftk.OpticalFlowAffineKlt, "lssd": ftk.OpticalFlowLssdKlt}[model]()
    flow.options().kMethod = method
    flow.options().kMaxTrackPointsNumber = max(slots, 500)
    kw = {} if epipolar_model is None else dict(epipolar_model=epipolar_model)
    tracker = ftk.KltVideoTracker(flow, slots, levels=K.LEVELS, min_distance=K.MIN_DISTANCE, min_response=K.MIN_RESPONSE, forward_backward=fb,
                                  epipolar_threshold=W.THRESHOLD, epipolar_hypotheses=hypotheses, epipolar_seed=W.SEED, **kw)
    states, fits, tracked_frames = [], [], 0
    for k, image in enumerate(W.frames(name)):
        if reset_before == k:
            tracker.reset()
            tracked_frames = 0
        started_from = tracker.points.cpu().numpy() if tracked_frames else None
        tracker.track(torch.from_numpy(image).cuda())
        states.append({t: getattr(tracker, t).cpu().numpy() for t in TENSORS})
        if tracked_frames:
            fit = {a: getattr(tracker, "epipolar_" + a) for a in ("F", "H", "best", "n_inliers", "model_chosen")}
            fits.append((tracker._st[0].cpu().numpy(), {a: None if t is None else t.cpu().numpy() for a, t in fit.items()}, started_from))
        tracked_frames += 1
    return tracker, states, fits


def _same_run(got, got_fits, want, want_fits, what):
    for k, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"{what}, frame {k}")
    assert len(got_fits) == len(want_fits)
    for k, ((_, after, fit, points), (status, held, got_points)) in enumerate(zip(want_fits, got_fits)):
        assert np.array_equal(status, after) and E.same(got_points, points), (what, k)
        assert int(held["model_chosen"][0]) == fit.model and E.same(held["best"], fit.best) and E.same(held["n_inliers"], fit.n_inliers), (what, k)
        assert E.same(held["F"], fit.F) and E.same(held["H"], fit.H), (what, k)


@pytest.mark.parametrize("epipolar_model", ["homography", "auto"])
@pytest.mark.parametrize("name", W.NAMES)
def test_every_frame_equals_the_restatement(ftk, oracle, name, epipolar_model):
    want, want_fits = W.reference_run(name, epipolar_model)
    _, got, got_fits = _run(ftk, name, epipolar_model)
    _same_run(got, got_fits, want, want_fits, f"{name}, {epipolar_model}")


def test_the_default_model_is_the_tracker_without_the_argument(ftk, oracle):
    tracker, explicit, explicit_fits = _run(ftk, "forward_backward", "fundamental")
    plain_tracker, plain, plain_fits = _run(ftk, "forward_backward", None)
    assert tracker.epipolar_H is None and tracker.epipolar_model_chosen is None and plain_tracker.epipolar_H is None
    assert tuple(tracker.epipolar_best.shape) == (1,) and "two_view" not in tracker._bound and "epipolar" in tracker._bound
    for k, (g, w) in enumerate(zip(explicit, plain)):
        _same(g, w, f"default model, frame {k}")
    for (status, held, _), (plain_status, plain_held, _) in zip(explicit_fits, plain_fits):
        assert np.array_equal(status, plain_status) and E.same(held["F"], plain_held["F"]) and E.same(held["best"], plain_held["best"])
    want, _ = V.reference_run("forward_backward")
    for k, (g, w) in enumerate(zip(plain, want)):
        _same(g, w, f"the fundamental route's restatement, frame {k}")


def test_on_one_plane_auto_retires_the_patch_where_the_fundamental_matrix_does_not(ftk, oracle):
    """"planar_patch": with "auto" every tracked track that starts at least 8 px inside the patch leaves the filter as LARGE_RESIDUAL and its
    slot retires, at most 1 in 20 background tracks does, the homography is chosen in every frame; "fundamental" on the same frames
    rejects strictly fewer patch tracks (on the CPU: 0 of 28 against 18 of 18)."""
    want, want_fits = W.reference_run("planar_patch", "auto")
    _, got, fits = _run(ftk, "planar_patch", "auto")
    _same_run(got, fits, want, want_fits, "planar_patch, auto")
    assert len(fits) == K.FRAMES - 1
    rejected_on = total_on = 0
    for k, (after, held, points) in enumerate(fits):
        before, ids = want_fits[k][0], got[k]["ids"]  # (the forward statuses before the filter are the oracle's: the device keeps only the filtered ones)
        on, off = V.on_patch(points) & (before == E.TRACKED), ~V.on_patch(points, -V.INSIDE) & (before == E.TRACKED)
        print(f"frame {k + 1}: {int(on.sum())} tracked on the patch, {int((after[on] == E.LARGE_RESIDUAL).sum())} rejected; "
              f"{int(off.sum())} off it, {int((after[off] == E.LARGE_RESIDUAL).sum())} rejected; model {held['model_chosen'][0]}, inliers {held['n_inliers']}")
        assert int(held["model_chosen"][0]) == 1
        assert on.sum() >= 2 and (after[on] == E.LARGE_RESIDUAL).all(), (k, after[on])
        assert off.sum() >= 90 and 20 * int((after[off] == E.LARGE_RESIDUAL).sum()) <= int(off.sum()), k
        assert not np.isin(ids[np.flatnonzero(on)], got[k + 1]["ids"]).any()  # the slots were emptied (and may hold fresh ids since)
        rejected_on, total_on = rejected_on + int(on.sum()), total_on + int(on.sum())
    want_f, want_fits_f = W.reference_run("planar_patch", "fundamental")
    _, got_f, fits_f = _run(ftk, "planar_patch", "fundamental")
    for k, (g, w) in enumerate(zip(got_f, want_f)):
        _same(g, w, f"planar_patch, fundamental, frame {k}")
    rejected_f = 0
    for k, (after, _, points) in enumerate(fits_f):
        on = V.on_patch(points) & (want_fits_f[k][0] == E.TRACKED)
        rejected_f += int((after[on] == E.LARGE_RESIDUAL).sum())
    print(f"patch tracks rejected: auto {rejected_on} of {total_on}, fundamental {rejected_f}")
    assert rejected_f < rejected_on


def test_on_depth_layers_auto_is_the_fundamental_route(ftk, oracle):
    want, want_fits = V.reference_run("moving_patch")
    _, got, fits = _run(ftk, "moving_patch", "auto")
    for k, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"moving_patch, auto, frame {k}")
    assert len(fits) == len(want_fits) == K.FRAMES - 1
    for (after, held, _), (_, want_after, best, n_inliers, _) in zip(fits, want_fits):
        assert int(held["model_chosen"][0]) == 0 and np.array_equal(after, want_after) and (int(held["best"][0]), int(held["n_inliers"][0])) == (best, n_inliers)


def test_reset_forgets_the_last_fit(ftk):
    import torch
    tracker = ftk.KltVideoTracker(ftk.OpticalFlowBasicKlt(), 64, levels=K.LEVELS, min_distance=K.MIN_DISTANCE, min_response=K.MIN_RESPONSE,
                                  epipolar_threshold=W.THRESHOLD, epipolar_hypotheses=128, epipolar_seed=W.SEED, epipolar_model="auto")
    for image in W.frames("basic_fast")[:2]:
        tracker.track(torch.from_numpy(image).cuda())
    assert int(tracker.epipolar_model_chosen.item()) >= 0 and bool((tracker.epipolar_F.any() | tracker.epipolar_H.any()).item())
    tracker.reset()
    assert int(tracker.epipolar_model_chosen.item()) == -1 and tracker.epipolar_best.tolist() == [-1, -1] and tracker.epipolar_n_inliers.tolist() == [0, 0]
    assert not bool(tracker.epipolar_F.any().item()) and not bool(tracker.epipolar_H.any().item())
