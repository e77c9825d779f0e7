"""The loud failures of the landmark table and ``TrackOdometry`` before any device is touched: the walk of
tests/args_walk.py over the two entries; the refusals of the entries, of ``TrackOdometry`` and of ``KltVideoTracker(odometry=...)``; the
agreement of header, library and binding; the plan walked through host/build/landmark_table_plan_cli."""
import types

import pytest

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402

K = (512.0, 512.0, 319.5, 239.5)


def _begin(w, n=40):
    from feature_tracker_amd import device as D
    return D.landmark_table_begin_device(w.ctx, w.t("ids", "int64", n), w.t("owner", "int64", n), w.t("landmarks", "float32", n, 3), w.t("anchor_frame", "int32", n),
                                         w.t("pnp_status", "uint8", n), w.t("anchor_status", "uint8", n), w.t("counters", "int32", 8))


def _end(w, n=40, K=K, threshold=1.0, c2=0.999, frame=3, mode=0, status=True, model=True):
    from feature_tracker_amd import device as D
    return D.landmark_table_end_device(w.ctx, w.t("ids", "int64", n), w.t("points", "float32", n, 2), w.t("status_in", "uint8", n) if status else None,
                                       w.t("pose_in", "float32", 7), w.t("valid_in", "int32", 1), w.t("model_in", "int32", 1) if model else None, frame, mode, K,
                                       threshold, c2, w.t("landmarks", "float32", n, 3), w.t("anchor_uv", "float32", n, 2), w.t("anchor_pose", "float32", n, 7),
                                       w.t("anchor_frame", "int32", n), w.t("counters", "int32", 8), w.t("pose", "float32", 7))


def test_entries_take_no_pointer_of_an_unchecked_argument(monkeypatch):
    A.walk_call(monkeypatch, _begin, ["ftk_landmark_table_begin_device"])
    A.walk_call(monkeypatch, _end, ["ftk_landmark_table_end_device"])
    A.walk_call(monkeypatch, lambda w: _end(w, mode=1, status=False, model=False), ["ftk_landmark_table_end_device"])


@pytest.mark.parametrize("kind", ["dtype", "shape", "device"])
def test_each_refused_tensor_stops_the_entries_before_the_library(monkeypatch, kind):
    # (ids with a row fewer is a valid tensor: the next one, sized by it, is the one refused)
    assert A.refusal_sweep(monkeypatch, _begin, kind, loose=("ids",)) == ["ids", "owner", "landmarks", "anchor_frame", "pnp_status", "anchor_status", "counters"]
    assert A.refusal_sweep(monkeypatch, _end, kind, loose=("ids",)) == ["ids", "points", "status_in", "pose_in", "valid_in", "model_in", "landmarks", "anchor_uv",
                                                                        "anchor_pose", "anchor_frame", "counters", "pose"]


def test_other_refusals(monkeypatch):
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    w = A.Walk(monkeypatch)
    nan, inf = float("nan"), float("inf")
    for match, kw in (("^K must be", dict(K=(0.0, 512.0, 319.5, 239.5))), ("^K must be", dict(K=(512.0, 512.0, nan, 1.0))), ("^K must be", dict(K=None)),
                      ("threshold", dict(threshold=-1.0)), ("threshold", dict(threshold=nan)), ("threshold", dict(threshold=2.0e19)),
                      ("^min_parallax_cos2 must be", dict(c2=-0.1)), ("^min_parallax_cos2 must be", dict(c2=1.5)), ("^min_parallax_cos2 must be", dict(c2=nan)),
                      ("^min_parallax_cos2 must be", dict(c2="narrow")), ("^frame must be", dict(frame=-1)), ("^frame must be", dict(frame=1 << 31)),
                      ("^mode must be", dict(mode=2)), ("integers", dict(frame="first")), ("^status_in must be given", dict(status=False)),
                      ("FTK_TRACK_TABLE_MAX_SLOTS", dict(n=65537))):
        with pytest.raises(ValueError, match=match):
            _end(w, **kw)
    with pytest.raises(ValueError, match="FTK_TRACK_TABLE_MAX_SLOTS"):
        _begin(w, n=65537)
    assert w.lib.calls == [] and w.unchecked_reads == []
    for kw in (dict(), dict(threshold=0.0), dict(c2=0.0), dict(c2=1.0), dict(frame=0), dict(frame=(1 << 31) - 1), dict(mode=1, status=False), dict(n=1), dict(n=65536)):
        _end(w, **kw)
    assert len(w.lib.calls) == 9
    recorder = A.RecorderLib()
    monkeypatch.setattr(N, "lib", lambda: recorder)
    for match, kw in (("^K must be", dict(K=(0.0, 1.0, 1.0, 1.0))), ("threshold", dict(K=K, threshold=-0.5)), ("baseline", dict(K=K, baseline=0.0)),
                      ("^min_parallax_deg must be", dict(K=K, min_parallax_deg=-1.0)), ("^min_parallax_deg must be", dict(K=K, min_parallax_deg=91.0)),
                      ("^min_parallax_deg must be", dict(K=K, min_parallax_deg=nan)), ("^min_parallax_deg must be", dict(K=K, min_parallax_deg=inf)),
                      ("^min_landmarks must be", dict(K=K, min_landmarks=5)), ("^min_landmarks must be", dict(K=K, min_landmarks=65537)),
                      ("^min_landmarks must be", dict(K=K, min_landmarks=30.0)), ("^hypotheses must be", dict(K=K, hypotheses=0)),
                      ("^refine_iterations must be", dict(K=K, refine_iterations=17)), ("^seed must be", dict(K=K, seed=-1)),
                      ("context_on_stream", dict(K=K, ctx=types.SimpleNamespace(handle=None)))):
        with pytest.raises(ValueError, match=match):
            F.TrackOdometry(**kw)
    odo = F.TrackOdometry(K)
    assert (odo.K, odo.threshold, odo.min_parallax_deg, odo.min_landmarks, odo.baseline, odo.hypotheses, odo.refine_iterations, odo.seed) == (K, 1.0, 1.0, 30, 1.0, 512, 4, 0)
    assert (odo.initialised, odo.frame) == (False, 0) and odo.reset() is odo
    ids, uv = torch.zeros(9, dtype=torch.int64), torch.zeros(9, 2)
    for match, args in (("^ids must be .*wrong dtype", (ids.int(), uv, (480, 640))), ("^points must be .*dimension 1 is 3", (ids, torch.zeros(9, 3), (480, 640))),
                        ("^image_size must be", (ids, uv, (0, 640))), ("^image_size must be", (ids, uv, None)), ("no CPU fallback", (ids, uv, (480, 640)))):
        with pytest.raises(ValueError, match=match):
            odo.update(*args)
    assert recorder.calls == [] and (odo.initialised, odo.frame) == (False, 0)
    # KltVideoTracker(odometry=...): a TrackOdometry on the tracker's own context, or a ValueError before any launch
    flow = F.OpticalFlowBasicKlt()
    ctx = types.SimpleNamespace(handle=None, stream=object(), device_index=0)
    other = types.SimpleNamespace(handle=None, stream=object(), device_index=1)
    for match, kw in (("^odometry must be a TrackOdometry or None", dict(odometry=object(), ctx=ctx)), ("^odometry must be a TrackOdometry built on", dict(odometry=odo, ctx=ctx)),
                      ("^odometry must be a TrackOdometry built on", dict(odometry=F.TrackOdometry(K, ctx=other), ctx=ctx)),
                      ("^odometry must be a TrackOdometry built on", dict(odometry=F.TrackOdometry(K, ctx=ctx)))):
        with pytest.raises(ValueError, match=match):
            F.KltVideoTracker(flow, 64, **kw)
    wired = F.TrackOdometry(K, ctx=ctx)
    assert F.KltVideoTracker(flow, 64, ctx=ctx, odometry=wired).odometry is wired and F.KltVideoTracker(flow, 64).odometry is None
    assert recorder.calls == []


def test_header_library_and_binding_agree():
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    names = ("BLOCK", "COUNTERS", "VALID", "N_NEW", "N_ANCHORED", "N_LANDMARKS", "N_DROPPED", "LOST", "STEADY", "BOOTSTRAP")
    header = A.header_library_and_binding_agree(tuple(f"FTK_LANDMARK_TABLE_{name}" for name in names), {"ftk_landmark_table_begin_device", "ftk_landmark_table_end_device"})
    assert "DESIGN.md 5.31" in header and "TrackOdometry" in F.__all__
    assert D.landmark_table_begin_device.__module__ == D.landmark_table_end_device.__module__ == "feature_tracker_amd._device_landmark_table"
    lib = N.lib()
    assert lib.ftk_landmark_table_begin_device(None, None, None, 8, None, None, None, None, None, None) == -1  # null context
    assert lib.ftk_landmark_table_end_device(None, None, None, None, 8, None, None, None, None, 0, 0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, None, None, None, None, None, None) == -1


def test_the_plan_walked_without_a_device():
    cases = [(n,) for n in (1, 63, 64, 65, 255, 256, 257, 1025, 65535, 65536)]
    refused = [((0,), "sizes"), ((-3,), "sizes"), ((65537,), "slots")]
    out = A.run_plan_tool(A.plan_cli("landmark_table_plan_cli"), cases + [c for c, _ in refused])
    for (n,), plan in zip(cases, out):
        assert plan == {"refused": "none", "launches": "1", "block": "256", "blocks": str(-(-n // 256)), "counters": "8"}
    for (_, name), plan in zip(refused, out[len(cases):]):
        assert plan == {"refused": name}


def test_nothing_in_the_package_imports_the_restatements():
    A.nothing_in_the_package_imports("track_odometry_ref")
    A.nothing_in_the_package_imports("landmark_table_ref")
