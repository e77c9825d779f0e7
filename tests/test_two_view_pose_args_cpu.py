"""The loud failures of TwoViewPose before any device is touched: the walk of tests/args_walk.py over
``device.two_view_pose_device``; the refusals of the entry, of ``TwoViewPose`` and of the library; the agreement of header, library and
binding; the workspace restated."""
import types

import pytest

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402

K = (512.0, 512.0, 319.5, 239.5)


def _call(w, n=40, K=K, K_cur=None, threshold=1.0, baseline=1.0):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    return D.two_view_pose_device(w.ctx, w.t("ref_uv", "float32", n, 2), w.t("cur_uv", "float32", n, 2), w.t("status", "uint8", n), K, K_cur, threshold, baseline,
                                  w.t("workspace", "int64", -(-N.two_view_pose_workspace_bytes(n) // 8)), w.t("pose", "float32", 7), w.t("points", "float32", n, 3),
                                  w.t("E", "float32", 3, 3), w.t("n_front", "int32", 4), w.t("valid", "int32", 1), w.t("n_points", "int32", 1))


def test_entry_takes_no_pointer_of_an_unchecked_argument(monkeypatch):
    A.walk_call(monkeypatch, _call, ["ftk_two_view_pose_device"])


@pytest.mark.parametrize("kind", ["dtype", "shape", "device"])
def test_each_refused_tensor_stops_the_entry_before_the_library(monkeypatch, kind):
    # (ref_uv with a row fewer is a valid tensor: cur_uv, sized by it, is the one refused)
    names = A.refusal_sweep(monkeypatch, _call, kind, loose=("ref_uv",))
    assert names == ["ref_uv", "cur_uv", "status", "workspace", "pose", "points", "E", "n_front", "valid", "n_points"]


def test_other_refusals(monkeypatch):
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    w = A.Walk(monkeypatch)
    nan, inf = float("nan"), float("inf")
    for match, kw in (("^K must be", dict(K=(0.0, 512.0, 319.5, 239.5))), ("^K must be", dict(K=(512.0, -1.0, 319.5, 239.5))), ("^K must be", dict(K=(nan, 512.0, 1.0, 1.0))),
                      ("^K must be", dict(K=(512.0, inf, 1.0, 1.0))), ("^K must be", dict(K=(512.0, 512.0, nan, 1.0))), ("^K must be", dict(K=(512.0, 512.0, 1.0))),
                      ("^K must be", dict(K=None)), ("^K_cur must be", dict(K_cur=(512.0, 0.0, 1.0, 1.0))), ("^K_cur must be", dict(K_cur=(512.0, 512.0, 1.0, -inf))),
                      ("^K_cur must be", dict(K_cur="camera")), ("threshold", dict(threshold=-1.0)), ("threshold", dict(threshold=nan)), ("threshold", dict(threshold=inf)),
                      ("threshold", dict(threshold="wide")), ("threshold", dict(threshold=2.0e19)),
                      ("^K must be", dict(K=(1e-50, 512.0, 1.0, 1.0))), ("^K must be", dict(K=(512.0, 1e39, 1.0, 1.0))), ("baseline", dict(baseline=1e-50)), ("baseline", dict(baseline=0.0)), ("baseline", dict(baseline=-0.1)), ("baseline", dict(baseline=nan)),
                      ("baseline", dict(baseline=inf)), ("FTK_TRACK_TABLE_MAX_SLOTS", dict(n=65537))):
        with pytest.raises(ValueError, match=match):
            _call(w, **kw)
    assert w.lib.calls == [] and w.unchecked_reads == []
    for kw in (dict(), dict(K_cur=(470.0, 455.0, 300.5, 251.25)), dict(threshold=0.0), dict(threshold=1.8e19), dict(baseline=0.12), dict(n=1), dict(n=65536)):
        _call(w, **kw)
    assert len(w.lib.calls) == 7
    recorder = A.RecorderLib()
    monkeypatch.setattr(N, "lib", lambda: recorder)
    for match, kw in (("^K must be", dict(K=(0.0, 1.0, 1.0, 1.0))), ("^K must be", dict(K=(1.0, 1.0))), ("^K_cur must be", dict(K=K, K_cur=(1.0, nan, 1.0, 1.0))),
                      ("threshold", dict(K=K, threshold=-0.5)), ("baseline", dict(K=K, baseline=0.0)), ("baseline", dict(K=K, baseline=inf)),
                      ("context_on_stream", dict(K=K, ctx=types.SimpleNamespace(handle=None)))):
        with pytest.raises(ValueError, match=match):
            F.TwoViewPose(**kw)
    pose = F.TwoViewPose(K)
    assert (pose.K, pose.K_cur, pose.threshold, pose.baseline) == (K, None, 1.0, 1.0)
    assert F.TwoViewPose([512, 512, 320, 240], K_cur=K, threshold=0, baseline=0.12).K == (512.0, 512.0, 320.0, 240.0)
    uv, st = torch.zeros(9, 2), torch.ones(9, dtype=torch.uint8)
    for match, args in (("^ref_uv must be .*wrong dtype", (uv.double(), uv, st)), ("^cur_uv must be .*dimension 1 is 3", (uv, torch.zeros(9, 3), st)),
                        ("^status must be .*wrong dtype", (uv, uv, st.bool())), ("no CPU fallback", (uv, uv, st))):
        with pytest.raises(ValueError, match=match):
            pose.solve(*args)
    assert recorder.calls == []


def test_header_library_and_binding_agree():
    import ctypes as C
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    header = A.header_library_and_binding_agree(("FTK_POSE_JACOBI_SWEEPS", "FTK_POSE_TILE"), {"ftk_two_view_pose_workspace_bytes", "ftk_two_view_pose_device"})
    assert header.count("ftk_two_view_pose_device below") == 2  # the two filters point here
    assert {"TwoViewPose", "TwoViewPoseResult"} <= set(F.__all__) and D.two_view_pose_device.__module__ == "feature_tracker_amd._device_two_view_pose"
    lib, out = N.lib(), C.c_int64()
    up16 = lambda v: (v + 15) & ~15  # noqa: E731
    for n in (1, 7, 8, 255, 256, 257, 1024, 1025, 65535, 65536):
        want = 16 + up16(16 * n) + up16(180 * -(-n // 256)) + 128  # csrc/two_view_pose_plan.cpp restated: M, the points, 45 totals per tile, the model block
        assert lib.ftk_two_view_pose_workspace_bytes(n, C.byref(out)) == 0 and out.value == N.two_view_pose_workspace_bytes(n) == want, n
    assert lib.ftk_two_view_pose_workspace_bytes(65537, C.byref(out)) == -4  # FTK_E_UNSUPPORTED
    assert lib.ftk_two_view_pose_workspace_bytes(0, C.byref(out)) == -1 and lib.ftk_two_view_pose_workspace_bytes(-1, C.byref(out)) == -1
    assert lib.ftk_two_view_pose_workspace_bytes(1, None) == -1
    assert lib.ftk_two_view_pose_device(None, None, None, None, None, 8, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, None, None, None, None, None, None, None) == -1  # null context


def test_nothing_in_the_package_imports_the_restatement():
    A.nothing_in_the_package_imports("two_view_pose_ref")
