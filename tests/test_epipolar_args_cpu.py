"""The loud failures of two-view outlier rejection before any device is touched: the walk of tests/args_walk.py
(duck-typed tensors, a recording stand-in for the native library) over ``device.epipolar_ransac_device``; the refusals of ``EpipolarRansac``
and of ``KltVideoTracker``'s new arguments; the agreement of header, library and binding; the launch plan through
host/build/epipolar_plan_cli; and the restated video run."""
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402

PLAN_CLI = A.plan_cli("epipolar_plan_cli")


def _call(w, n=40, k=64, image=(120, 160), threshold=1.0, seed=0):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    return D.epipolar_ransac_device(w.ctx, w.t("ref_uv", "float32", n, 2), w.t("cur_uv", "float32", n, 2), w.t("status", "uint8", n), image, threshold, k, seed,
                                    w.t("workspace", "int64", -(-N.epipolar_workspace_bytes(n, k) // 8)), w.t("best", "int32", 1), w.t("n_inliers", "int32", 1),
                                    w.t("F", "float32", 3, 3), w.t("counts", "int32", k), w.t("models", "float32", k, 9))


def test_entry_takes_no_pointer_of_an_unchecked_argument(monkeypatch):
    A.walk_call(monkeypatch, _call, ["ftk_epipolar_ransac_device"])


@pytest.mark.parametrize("kind", ["dtype", "shape", "device"])
def test_each_refused_tensor_stops_the_entry_before_the_library(monkeypatch, kind):
    # (ref_uv with a row fewer is a valid tensor: cur_uv, sized by it, is the one refused)
    A.refusal_sweep(monkeypatch, _call, kind, loose=("ref_uv",))


def test_other_refusals(monkeypatch):
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    w = A.Walk(monkeypatch)
    for match, kw in (("hypotheses must be in 1 .. FTK_EPIPOLAR_MAX_HYPOTHESES", dict(k=4097)), ("hypotheses must be", dict(k=0)), ("threshold", dict(threshold=-1.0)),
                      ("threshold", dict(threshold=float("nan"))), ("threshold", dict(threshold=float("inf"))), ("image_size", dict(image=(0, 160))),
                      ("image_size", dict(image=(120,))), ("image_size", dict(image=(70000, 160))), ("seed must be a uint32", dict(seed=-1)),
                      ("seed must be a uint32", dict(seed=1 << 32)), ("FTK_TRACK_TABLE_MAX_SLOTS", dict(n=65537))):
        with pytest.raises(ValueError, match=match):
            _call(w, **kw)
    assert w.lib.calls == [] and w.unchecked_reads == []
    recorder = A.RecorderLib()
    monkeypatch.setattr(N, "lib", lambda: recorder)
    for match, kw in (("hypotheses", dict(hypotheses=0)), ("hypotheses", dict(hypotheses=4097)), ("threshold", dict(threshold=-0.5)), ("seed", dict(seed=-3)),
                      ("context_on_stream", dict(ctx=types.SimpleNamespace(handle=None)))):
        with pytest.raises(ValueError, match=match):
            F.EpipolarRansac(**kw)
    ransac = F.EpipolarRansac()
    assert (ransac.hypotheses, ransac.threshold, ransac.seed) == (512, 1.0, 0)
    uv, st = torch.zeros(9, 2), torch.ones(9, dtype=torch.uint8)
    for match, args in (("^ref_uv must be .*wrong dtype", (uv.double(), uv, st)), ("^cur_uv must be .*dimension 1 is 3", (uv, torch.zeros(9, 3), st)),
                        ("^status must be .*wrong dtype", (uv, uv, st.bool())), ("^ref_uv must be a torch tensor", (uv.numpy(), uv, st)),
                        (r"pass cur_uv\.contiguous\(\)", (uv, torch.zeros(9, 4)[:, ::2], st)), ("no CPU fallback", (uv, uv, st))):
        with pytest.raises(ValueError, match=match):
            ransac.filter(*args, (120, 160))
    with pytest.raises(ValueError, match="image_size"):
        ransac.filter(uv, uv, st, (120, 0))
    flow = F.OpticalFlowBasicKlt()
    for match, kw in (("threshold", dict(epipolar_threshold=-1.0)), ("threshold", dict(epipolar_threshold=float("nan"))),
                      ("hypotheses", dict(epipolar_threshold=1.0, epipolar_hypotheses=0)), ("seed", dict(epipolar_threshold=1.0, epipolar_seed=-1))):
        with pytest.raises(ValueError, match=match):
            F.KltVideoTracker(flow, 8, **kw)
    tracker = F.KltVideoTracker(flow, 8, epipolar_hypotheses=0)  # without a threshold the other two are not read
    assert tracker.epipolar_threshold is None and tracker.epipolar_F is None
    assert F.KltVideoTracker(flow, 8, epipolar_threshold=0.5).epipolar_hypotheses == 512
    assert recorder.calls == []


def test_header_library_and_binding_agree():
    import ctypes as C
    from feature_tracker_amd import _native as N
    A.header_library_and_binding_agree(("FTK_EPIPOLAR_MAX_HYPOTHESES", "FTK_EPIPOLAR_SAMPLE", "FTK_EPIPOLAR_MAX_ATTEMPTS", "FTK_EPIPOLAR_SCORE_TILE"),
                                       {"ftk_epipolar_workspace_bytes", "ftk_epipolar_ransac_device"})
    lib, out = N.lib(), C.c_int64()
    for n, k in ((1, 1), (7, 3), (300, 512), (1025, 1000), (65536, 4096)):
        assert lib.ftk_epipolar_workspace_bytes(n, k, C.byref(out)) == 0 and out.value == N.epipolar_workspace_bytes(n, k)
    assert lib.ftk_epipolar_workspace_bytes(65537, 1, C.byref(out)) == -4 and lib.ftk_epipolar_workspace_bytes(1, 4097, C.byref(out)) == -4  # FTK_E_UNSUPPORTED
    assert lib.ftk_epipolar_workspace_bytes(0, 1, C.byref(out)) == -1 and lib.ftk_epipolar_workspace_bytes(1, 0, C.byref(out)) == -1
    assert lib.ftk_epipolar_workspace_bytes(1, 1, None) == -1
    assert lib.ftk_epipolar_ransac_device(None, None, None, None, None, 8, 1, 1, 1.0, 1, 0, None, None, None, None, None, None) == -1  # null context


def test_nothing_in_the_package_imports_the_restatement():
    A.nothing_in_the_package_imports("epipolar_ref")


def _plan(n, k, rows, cols):
    """The plan restated (csrc/two_view_plan.cpp with one slot)."""
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
    off_models = off_counts + up16(4 * k)
    off_valid = off_models + up16(36 * k)
    return {"refused": "none", "scan_block": 1024, "scan_per_thread": -(-n // 1024), "scan_lds": 4096, "hyp_block": 64, "hyp_blocks": -(-k // 64),
            "hyp_lds": 90 * 64 * 4, "score_tile": 256, "score_group": 16, "score_tiles": -(-n // 256), "score_groups": -(-k // 16), "score_lds": 4096,
            "select_per_thread": -(-k // 1024), "off_points": off_points, "off_list": off_list, "off_counts": off_counts, "off_models": off_models,
            "off_valid": off_valid, "bytes": off_valid + up16(k)}


def test_plan_cli_equals_the_restated_plan():
    from feature_tracker_amd import _native as N
    cases = [(n, k, 480, 640) for n in (0, 1, 7, 256, 257, 1024, 1025, 65536, 65537, -1) for k in (0, 1, 16, 17, 64, 65, 1024, 1025, 4096, 4097)]
    cases += [(8, 8, 0, 640), (8, 8, 480, 65537), (8, 8, 65536, 65536)]
    plans = A.run_plan_tool(PLAN_CLI, cases)
    seen = set()
    for case, got in zip(cases, plans):
        want = _plan(*case)
        assert got == {k: str(v) for k, v in want.items()}, (case, got, want)
        seen.add(want["refused"])
        if want["refused"] == "none":
            assert want["bytes"] == N.epipolar_workspace_bytes(case[0], case[1]) and want["scan_per_thread"] <= 64
    assert seen == {"none", "sizes", "points", "hypotheses"}


def test_the_restated_video_run_rejects_tracks_and_changes_the_tables():
    """tests/klt_video_epipolar_cases.py on the CPU: the filter between the forward and the backward call rejects tracked slots, they retire
    with LARGE_RESIDUAL, and the tables differ from the run without it (tests/klt_video_cases.py)."""
    from tests import epipolar_ref as E
    from tests import klt_video_cases as K
    from tests import klt_video_epipolar_cases as V
    states, fits = V.reference_run("forward_backward")
    plain, _ = K.reference_run("forward_backward")
    rejected = sum(int(((before == E.TRACKED) & (after == E.LARGE_RESIDUAL)).sum()) for before, after, _, _, _ in fits)
    assert rejected >= 1 and all(best >= 0 for _, _, best, _, _ in fits)
    assert any(not np.array_equal(a["ids"], b["ids"]) for a, b in zip(states, plain))
    for before, after, _, n_inliers, _ in fits:
        assert (after[before != E.TRACKED] == before[before != E.TRACKED]).all() and n_inliers == int((after == E.TRACKED).sum())


def test_the_restated_moving_patch_retires_its_tracks():
    """The "moving_patch" sequence on the CPU (tests/test_klt_video_epipolar_gpu.py holds the device to the same run): in every frame every
    tracked track on the patch is rejected, none off it is, and the flows are what the sequence was built to show."""
    from tests import klt_video_epipolar_cases as V
    _, fits = V.reference_run("moving_patch")
    assert len(fits) == 4
    for before, after, best, _, points in fits:
        on, rejected_on, off, rejected_off = V.patch_verdict(before, after, points)
        assert best >= 0 and on >= 3 and rejected_on == on and off >= 90 and rejected_off == 0, (on, rejected_on, off, rejected_off)
