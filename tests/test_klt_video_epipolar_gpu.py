"""KltVideoTracker with ``epipolar_threshold`` on the device against its restatement (tests/klt_video_epipolar_cases.py: the track table's
and the epipolar restatements composed with the oracle's trackers): after every frame all seven tensors of the table are
equal bit for bit, with and without the forward-backward check, and in a sequence where a patch of the image moves against the rest the
tracks on it retire with LARGE_RESIDUAL."""
import numpy as np
import pytest

from tests import epipolar_ref as E
from tests import klt_video_cases as K
from tests import klt_video_epipolar_cases as V
from tests.test_klt_video_gpu import TENSORS, _same

pytestmark = pytest.mark.gpu


def _run(ftk, name, filtered=True):
    """The device tracker over the case's frames: per frame a host copy of the seven tensors, and per tracked frame the fit it holds, its
    own forward statuses after the filter and the points the frame started from."""
    import torch
    model, method, slots, fb, reset_before, hypotheses, _ = V.config(name)
    flow = {"basic": ftk.OpticalFlowBasicKlt, "affine": ftk.OpticalFlowAffineKlt, "lssd": ftk.OpticalFlowLssdKlt}[model]()
    flow.options().kMethod = method
    flow.options().kMaxTrackPointsNumber = max(slots, 500)
    kw = dict(epipolar_threshold=V.THRESHOLD, epipolar_hypotheses=hypotheses, epipolar_seed=V.SEED) if filtered else {}
    tracker = ftk.KltVideoTracker(flow, slots, levels=K.LEVELS, min_distance=K.MIN_DISTANCE, min_response=K.MIN_RESPONSE, forward_backward=fb, **kw)
    states, fits, tracked_frames = [], [], 0
    for k, image in enumerate(V.frames(name)):
        if reset_before == k:
            tracker.reset()
            tracked_frames = 0
        started_from = tracker.points.cpu().numpy() if tracked_frames else None
        tracker.track(torch.from_numpy(image).cuda())
        states.append({t: getattr(tracker, t).cpu().numpy() for t in TENSORS})
        if tracked_frames and filtered:
            fits.append((tracker._st[0].cpu().numpy(), int(tracker.epipolar_best.item()), int(tracker.epipolar_n_inliers.item()), started_from))
        tracked_frames += 1
    return tracker, states, fits


@pytest.mark.parametrize("name", V.NAMES)
def test_every_frame_equals_the_restatement(ftk, oracle, name):
    want, want_fits = V.reference_run(name)
    _, got, got_fits = _run(ftk, name)
    for k, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"{name}, frame {k}")
    assert len(got_fits) == len(want_fits)
    for k, ((_, after, best, n_inliers, points), (status, got_best, got_inliers, got_points)) in enumerate(zip(want_fits, got_fits)):
        assert (got_best, got_inliers) == (best, n_inliers) and np.array_equal(status, after) and E.same(got_points, points), (name, k)


def test_tracks_on_a_patch_that_moves_against_the_rest_retire_with_large_residual(ftk, oracle):
    """Every track that starts on the patch and is tracked forward leaves the filter as LARGE_RESIDUAL, in every frame, and its slot
    retires: the id it held is gone from the table.  The rest of the image (four depth layers) is left alone: the filter rejects none of
    the tracks off the patch.  All of it on the device's own tensors, which also equal the restatement bit for bit."""
    want, want_fits = V.reference_run("moving_patch")
    _, got, fits = _run(ftk, "moving_patch")
    for k, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"moving_patch, frame {k}")
    assert len(fits) == K.FRAMES - 1
    for k, (after, best, n_inliers, points) in enumerate(fits):
        before, held = want_fits[k][0], got[k]["ids"]  # (the forward statuses before the filter are the oracle's: the device keeps only the filtered ones)
        on, off = V.on_patch(points) & (before == E.TRACKED), ~V.on_patch(points, -V.INSIDE) & (before == E.TRACKED)
        print(f"frame {k + 1}: {int(on.sum())} tracked on the patch, {int((after[on] == E.LARGE_RESIDUAL).sum())} rejected; "
              f"{int(off.sum())} off it, {int((after[off] == E.LARGE_RESIDUAL).sum())} rejected; best {best}, {n_inliers} inliers")
        assert on.sum() >= 3 and (after[on] == E.LARGE_RESIDUAL).all(), (k, after[on])
        assert best >= 0 and off.sum() >= 90 and (after[off] == E.TRACKED).all(), (k, int((after[off] != E.TRACKED).sum()))
        now = got[k + 1]
        retired = np.flatnonzero(on)
        assert not np.isin(held[retired], now["ids"]).any()  # the slots were emptied (and may hold fresh ids since)
        kept = np.flatnonzero(off)
        assert np.array_equal(now["ids"][kept], held[kept])


def test_without_a_threshold_the_tracker_is_the_one_it_was(ftk, oracle):
    plain, _ = K.reference_run("forward_backward")
    tracker, got, _ = _run(ftk, "forward_backward", filtered=False)
    assert tracker.epipolar_F is None and tracker.epipolar_threshold is None
    for k, (g, w) in enumerate(zip(got, plain)):
        _same(g, w, f"no filter, frame {k}")


def test_reset_forgets_the_last_fit(ftk):
    import torch
    _, _, _, _, _, hypotheses, _ = V.config("basic_fast")
    flow = ftk.OpticalFlowBasicKlt()
    tracker = ftk.KltVideoTracker(flow, 64, levels=K.LEVELS, min_distance=K.MIN_DISTANCE, min_response=K.MIN_RESPONSE, epipolar_threshold=V.THRESHOLD,
                                  epipolar_hypotheses=hypotheses, epipolar_seed=V.SEED)
    for image in V.frames("basic_fast")[:2]:
        tracker.track(torch.from_numpy(image).cuda())
    assert int(tracker.epipolar_best.item()) >= 0 and bool(tracker.epipolar_F.any().item())
    tracker.reset()
    assert int(tracker.epipolar_best.item()) == -1 and int(tracker.epipolar_n_inliers.item()) == 0 and not bool(tracker.epipolar_F.any().item())
