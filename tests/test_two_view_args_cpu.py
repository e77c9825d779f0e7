"""The loud failures of two-view outlier rejection with a choice of model before any device is touched: the walk of
tests/args_walk.py over ``device.two_view_ransac_device``; the refusals of ``TwoViewRansac`` and of ``KltVideoTracker``'s new
arguments; the agreement of header, library and binding; the launch plan through host/build/two_view_plan_cli; and the restated video runs."""
import types

import pytest

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402

PLAN_CLI = A.plan_cli("two_view_plan_cli")


def _call(w, n=40, k=64, image=(120, 160), threshold=1.0, seed=0, model="auto", permille=750):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    return D.two_view_ransac_device(w.ctx, w.t("ref_uv", "float32", n, 2), w.t("cur_uv", "float32", n, 2), w.t("status", "uint8", n), image, threshold, k, seed,
                                    model, permille, w.t("workspace", "int64", -(-N.two_view_workspace_bytes(n, k) // 8)), w.t("model_out", "int32", 1),
                                    w.t("best", "int32", 2), w.t("n_inliers", "int32", 2), w.t("F", "float32", 3, 3), w.t("H", "float32", 3, 3),
                                    w.t("counts", "int32", 2, k), w.t("models", "float32", 2, k, 9))


def test_entry_takes_no_pointer_of_an_unchecked_argument(monkeypatch):
    A.walk_call(monkeypatch, _call, ["ftk_two_view_ransac_device"])


@pytest.mark.parametrize("kind", ["dtype", "shape", "device"])
def test_each_refused_tensor_stops_the_entry_before_the_library(monkeypatch, kind):
    # (ref_uv with a row fewer is a valid tensor: cur_uv, sized by it, is the one refused)
    A.refusal_sweep(monkeypatch, _call, kind, loose=("ref_uv",))


def test_other_refusals(monkeypatch):
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    w = A.Walk(monkeypatch)
    for match, kw in (("hypotheses must be in 1 .. FTK_EPIPOLAR_MAX_HYPOTHESES", dict(k=4097)), ("threshold", dict(threshold=-1.0)),
                      ("image_size", dict(image=(0, 160))), ("seed must be a uint32", dict(seed=-1)), ("FTK_TRACK_TABLE_MAX_SLOTS", dict(n=65537)),
                      ("model must be one of", dict(model="affine")), ("model must be one of", dict(model=3)), ("model must be one of", dict(model=None)),
                      ("prefer_homography_permille", dict(permille=1001)), ("prefer_homography_permille", dict(permille=-1)),
                      ("prefer_homography_permille", dict(permille=0.75))):
        with pytest.raises(ValueError, match=match):
            _call(w, **kw)
    assert w.lib.calls == [] and w.unchecked_reads == []
    for model in ("fundamental", "homography", "auto", 0, 1, 2):
        _call(w, model=model)
    assert len(w.lib.calls) == 6
    recorder = A.RecorderLib()
    monkeypatch.setattr(N, "lib", lambda: recorder)
    for match, kw in (("model must be one of", dict(model="essential")), ("model must be one of", dict(model=None)), ("hypotheses", dict(hypotheses=0)),
                      ("threshold", dict(threshold=-0.5)), ("seed", dict(seed=-3)), ("prefer_homography", dict(prefer_homography=1.001)),
                      ("prefer_homography", dict(prefer_homography=-0.1)), ("prefer_homography", dict(prefer_homography=float("nan"))),
                      ("prefer_homography", dict(prefer_homography=float("inf"))), ("prefer_homography", dict(prefer_homography="much")),
                      ("context_on_stream", dict(ctx=types.SimpleNamespace(handle=None)))):
        with pytest.raises(ValueError, match=match):
            F.TwoViewRansac(**kw)
    ransac = F.TwoViewRansac()
    assert (ransac.model, ransac.mode, ransac.hypotheses, ransac.threshold, ransac.prefer_homography_permille, ransac.seed) == ("auto", 2, 512, 1.0, 750, 0)
    assert [F.TwoViewRansac(prefer_homography=x).prefer_homography_permille for x in (0, 1, 0.0004, 0.0006, 0.9996)] == [0, 1000, 0, 1, 1000]
    uv, st = torch.zeros(9, 2), torch.ones(9, dtype=torch.uint8)
    for match, args in (("^ref_uv must be .*wrong dtype", (uv.double(), uv, st)), ("^cur_uv must be .*dimension 1 is 3", (uv, torch.zeros(9, 3), st)),
                        ("^status must be .*wrong dtype", (uv, uv, st.bool())), ("no CPU fallback", (uv, uv, st))):
        with pytest.raises(ValueError, match=match):
            ransac.filter(*args, (120, 160))
    with pytest.raises(ValueError, match="image_size"):
        ransac.filter(uv, uv, st, (120, 0))
    flow = F.OpticalFlowBasicKlt()
    for match, kw in (("needs epipolar_threshold", dict(epipolar_model="auto")), ("needs epipolar_threshold", dict(epipolar_model="homography")),
                      ("model must be one of", dict(epipolar_threshold=1.0, epipolar_model="essential")),
                      ("epipolar_model must be", dict(epipolar_threshold=1.0, epipolar_model=2)),
                      ("prefer_homography", dict(epipolar_threshold=1.0, epipolar_model="auto", epipolar_prefer_homography=2.0))):
        with pytest.raises(ValueError, match=match):
            F.KltVideoTracker(flow, 8, **kw)
    tracker = F.KltVideoTracker(flow, 8, epipolar_threshold=0.5)
    assert tracker.epipolar_model == "fundamental" and tracker.epipolar_H is None and tracker.epipolar_model_chosen is None
    assert F.KltVideoTracker(flow, 8, epipolar_threshold=0.5, epipolar_model="auto").epipolar_model == "auto"
    assert F.KltVideoTracker(flow, 8).epipolar_model == "fundamental"
    assert recorder.calls == []


def test_header_library_and_binding_agree():
    import ctypes as C
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    A.header_library_and_binding_agree(("FTK_TWO_VIEW_FUNDAMENTAL", "FTK_TWO_VIEW_HOMOGRAPHY", "FTK_TWO_VIEW_AUTO", "FTK_TWO_VIEW_HOMOGRAPHY_SAMPLE"),
                                       {"ftk_two_view_workspace_bytes", "ftk_two_view_ransac_device"})
    assert N.TWO_VIEW_MODES == {"fundamental": N.FTK_TWO_VIEW_FUNDAMENTAL, "homography": N.FTK_TWO_VIEW_HOMOGRAPHY, "auto": N.FTK_TWO_VIEW_AUTO}
    assert {"TwoViewRansac", "TwoViewResult"} <= set(F.__all__)
    lib, out = N.lib(), C.c_int64()
    for n, k in ((1, 1), (7, 3), (300, 512), (1025, 1000), (65536, 4096)):
        for mode in (0, 1, 2):
            assert lib.ftk_two_view_workspace_bytes(n, k, mode, C.byref(out)) == 0 and out.value == N.two_view_workspace_bytes(n, k, mode)
    assert lib.ftk_two_view_workspace_bytes(65537, 1, 2, C.byref(out)) == -4 and lib.ftk_two_view_workspace_bytes(1, 4097, 2, C.byref(out)) == -4  # FTK_E_UNSUPPORTED
    assert lib.ftk_two_view_workspace_bytes(0, 1, 2, C.byref(out)) == -1 and lib.ftk_two_view_workspace_bytes(1, 0, 2, C.byref(out)) == -1
    assert lib.ftk_two_view_workspace_bytes(1, 1, 3, C.byref(out)) == -1 and lib.ftk_two_view_workspace_bytes(1, 1, -1, C.byref(out)) == -1
    assert lib.ftk_two_view_workspace_bytes(1, 1, 2, None) == -1
    assert lib.ftk_two_view_ransac_device(None, None, None, None, None, 8, 1, 1, 1.0, 1, 0, 2, 750, None, None, None, None, None, None, None, None) == -1  # null context


def test_nothing_in_the_package_imports_the_restatement():
    A.nothing_in_the_package_imports("two_view_ref")


def _plan(n, k, rows, cols, mode, permille):
    """The plan restated (csrc/two_view_plan.cpp)."""
    if not 0 <= mode <= 2:
        return {"refused": "mode"}
    if not 0 <= permille <= 1000:
        return {"refused": "prefer"}
    if n < 1 or k < 1 or not 1 <= rows <= 65536 or not 1 <= cols <= 65536:
        return {"refused": "sizes"}
    if n > 65536:
        return {"refused": "points"}
    if k > 4096:
        return {"refused": "hypotheses"}
    up16 = lambda v: (v + 15) & ~15  # noqa: E731
    off_points = 16
    off_list = off_points + up16(16 * n)
    off_counts = off_list + up16(4 * n)
    off_models = off_counts + up16(8 * k)
    off_valid = off_models + up16(72 * k)
    run_f, run_h = int(mode != 1), int(mode != 0)
    return {"refused": "none", "run_fundamental": run_f, "run_homography": run_h, "launches": 2 + 2 * (run_f + run_h), "scan_block": 1024,
            "scan_per_thread": -(-n // 1024), "hyp_block": 64, "hyp_blocks": -(-k // 64), "hyp_lds": 90 * 64 * 4, "score_tile": 256, "score_group": 16,
            "score_tiles": -(-n // 256), "score_groups": -(-k // 16), "score_lds": 4096, "select_per_thread": -(-k // 1024), "off_points": off_points,
            "off_list": off_list, "off_counts": off_counts, "off_models": off_models, "off_valid": off_valid, "bytes": off_valid + up16(2 * k)}


def test_plan_cli_equals_the_restated_plan():
    from feature_tracker_amd import _native as N
    cases = [(n, k, 480, 640, mode, 750) for n in (0, 1, 3, 4, 7, 8, 256, 257, 1024, 1025, 65536, 65537, -1) for k in (0, 1, 16, 17, 64, 65, 1024, 1025, 4096, 4097)
             for mode in (0, 1, 2)]
    cases += [(8, 8, 0, 640, 2, 750), (8, 8, 480, 65537, 2, 750), (8, 8, 65536, 65536, 2, 750), (8, 8, 480, 640, 3, 750), (8, 8, 480, 640, -1, 750),
              (8, 8, 480, 640, 2, -1), (8, 8, 480, 640, 2, 1001), (8, 8, 480, 640, 2, 0), (8, 8, 480, 640, 2, 1000)]
    plans = A.run_plan_tool(PLAN_CLI, cases)
    seen = set()
    for case, got in zip(cases, plans):
        want = _plan(*case)
        assert got == {k: str(v) for k, v in want.items()}, (case, got, want)
        seen.add(want["refused"])
        if want["refused"] == "none":
            assert want["bytes"] == N.two_view_workspace_bytes(case[0], case[1], case[4]) and want["scan_per_thread"] <= 64
            assert want["bytes"] >= N.epipolar_workspace_bytes(case[0], case[1])
    assert seen == {"none", "sizes", "points", "hypotheses", "mode", "prefer"}


def test_the_restated_planar_patch_retires_its_tracks_under_auto_and_not_under_the_fundamental_matrix():
    """The "planar_patch" sequence on the CPU (tests/test_klt_video_two_view_gpu.py holds the device to the same runs): under "auto" the
    homography is chosen in every frame, every tracked track on the patch is rejected and at most 1 in 20 off it; the fundamental matrix on
    the same frames rejects strictly fewer patch tracks.  Measured: auto 18 of 18 on the patch and 0 off it, fundamental 0 of 28."""
    from tests import klt_video_two_view_cases as W
    _, fits = W.reference_run("planar_patch", "auto")
    assert len(fits) == 4
    rejected = 0
    for (on, rejected_on, off, rejected_off), (_, _, fit, _) in zip(W.verdicts(fits), fits):
        assert fit.model == 1 and on >= 2 and rejected_on == on and off >= 90 and 20 * rejected_off <= off, (on, rejected_on, off, rejected_off)
        rejected += rejected_on
    _, fits_f = W.reference_run("planar_patch", "fundamental")
    rejected_f = sum(v[1] for v in W.verdicts(fits_f))
    print(f"patch tracks rejected: auto {rejected}, fundamental {rejected_f} of {sum(v[0] for v in W.verdicts(fits_f))}")
    assert rejected_f < rejected


def test_the_restated_depth_layers_keep_the_fundamental_matrix_under_auto():
    from tests import epipolar_ref as E
    from tests import klt_video_epipolar_cases as V
    from tests import klt_video_two_view_cases as W
    states, fits = W.reference_run("moving_patch", "auto")
    want_states, want_fits = V.reference_run("moving_patch")
    assert all(fit.model == 0 for _, _, fit, _ in fits)
    for (_, after, fit, _), (_, want_after, best, n_inliers, _) in zip(fits, want_fits):
        assert E.same(after, want_after) and (int(fit.best[0]), int(fit.n_inliers[0])) == (best, n_inliers)
    for a, b in zip(states, want_states):
        assert all(E.same(a[t], b[t]) for t in a)
