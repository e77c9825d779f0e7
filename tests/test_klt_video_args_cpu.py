"""The loud failures of masked Harris detection, the track-table entries and ``KltVideoTracker`` before any device is touched (DESIGN.md
5.19): the walk of tests/args_walk.py (duck-typed tensors, a recording stand-in for the native library) over the new entries of
device.py; the agreement of header, library and binding; and the launch plan through host/build/track_table_plan_cli."""
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402

PLAN_CLI = A.plan_cli("track_table_plan_cli")


class _Pyramid:
    handle = None

    def __init__(self, rows=120, cols=160):
        self.rows, self.cols = rows, cols

    def level_desc(self, i):
        return 0, self.rows, self.cols


def _detect(w, pyr=None, max_count=8, distance=9):
    from feature_tracker_amd import device as D
    return D.harris_detect_device(w.ctx, pyr or _Pyramid(), max_count, distance, 40.0, w.t("uv_out", "float32", max_count, 2), w.t("count_out", "int32", 1),
                                  w.t("occupied", "float32", 5, 2), w.t("occupied_mask", "uint8", 5))


def _table(w, n=6):
    return [w.t("ids", "int64", n), w.t("points", "float32", n, 2), w.t("prev_points", "float32", n, 2), w.t("status", "uint8", n), w.t("age", "int32", n),
            w.t("n_live", "int32", 1)]


def _retire(w, n=6):
    from feature_tracker_amd import device as D
    return D.track_table_retire_device(w.ctx, *_table(w, n), w.t("tracked_uv", "float32", n, 2), w.t("tracked_status", "uint8", n), w.t("free_slots", "int32", n),
                                       w.t("n_free", "int32", 1), w.t("back_uv", "float32", n, 2), w.t("back_status", "uint8", n), 1.0)


def _fill(w, n=6, pyr=None):
    from feature_tracker_amd import device as D
    return D.track_table_fill_device(w.ctx, pyr or _Pyramid(), 9, 40.0, *_table(w, n), w.t("next_id", "int64", 1), w.t("free_slots", "int32", n),
                                     w.t("n_free", "int32", 1))


CALLS = {"ftk_harris_detect_device": _detect, "ftk_track_table_retire_device": _retire, "ftk_track_table_fill_device": _fill}


@pytest.mark.parametrize("native", sorted(CALLS))
def test_entries_take_no_pointer_of_an_unchecked_argument(monkeypatch, native):
    A.walk_call(monkeypatch, CALLS[native], [native])


@pytest.mark.parametrize("native", sorted(CALLS))
@pytest.mark.parametrize("kind", ["dtype", "shape", "device"])
def test_each_refused_tensor_stops_the_entry_before_the_library(monkeypatch, native, kind):
    """Every tensor argument of every entry in turn with another dtype, one element too many in its first dimension, or on another device."""
    # (ids and occupied are the tensors the others are sized by: the NEXT one is refused)
    A.refusal_sweep(monkeypatch, CALLS[native], kind, loose=("ids", "occupied"), reshape=A.one_row_more)


def test_other_refusals_of_the_entries(monkeypatch):
    from feature_tracker_amd import device as D
    w = A.Walk(monkeypatch)
    with pytest.raises(ValueError, match="FTK_HARRIS_DEVICE_MAX_SURVIVORS"):
        _detect(w, _Pyramid(257, 256), distance=1)  # 65 792 cells
    with pytest.raises(ValueError, match="FTK_HARRIS_DEVICE_MAX_SURVIVORS"):
        D.track_table_fill_device(w.ctx, _Pyramid(600, 600), 2, 40.0,  # 300 x 300 cells
            *_table(w), w.t("next_id", "int64", 1), w.t("free_slots", "int32", 6), w.t("n_free", "int32", 1))
    with pytest.raises(ValueError, match="must not be negative"):
        D.harris_detect_device(w.ctx, _Pyramid(), -1, 9, 40.0, w.t("uv_out", "float32", 0, 2), w.t("count_out", "int32", 1))
    with pytest.raises(ValueError, match="occupied_mask without occupied"):
        D.harris_detect_device(w.ctx, _Pyramid(), 4, 9, 40.0, w.t("uv_out", "float32", 4, 2), w.t("count_out", "int32", 1), None, w.t("occupied_mask", "uint8", 5))
    with pytest.raises(ValueError, match="go together"):
        D.track_table_retire_device(w.ctx, *_table(w), w.t("tracked_uv", "float32", 6, 2), w.t("tracked_status", "uint8", 6), w.t("free_slots", "int32", 6),
                                    w.t("n_free", "int32", 1), w.t("back_uv", "float32", 6, 2))
    with pytest.raises(ValueError, match="fb_threshold"):
        D.track_table_retire_device(w.ctx, *_table(w), w.t("tracked_uv", "float32", 6, 2), w.t("tracked_status", "uint8", 6), w.t("free_slots", "int32", 6),
                                    w.t("n_free", "int32", 1), w.t("back_uv", "float32", 6, 2), w.t("back_status", "uint8", 6), float("nan"))
    with pytest.raises(ValueError, match="1 .. 65536 slots"):
        D.track_table_retire_device(w.ctx, *_table(w, 65537), w.t("tracked_uv", "float32", 65537, 2), w.t("tracked_status", "uint8", 65537),
                                    w.t("free_slots", "int32", 65537), w.t("n_free", "int32", 1))
    assert w.lib.calls == [] and w.unchecked_reads == []
    # strides and host tensors, on real CPU tensors
    ctx = types.SimpleNamespace(handle=None)
    with pytest.raises(ValueError, match="^uv_out must be a CUDA tensor"):
        D.harris_detect_device(ctx, _Pyramid(), 4, 9, 40.0, torch.zeros(4, 2), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"pass uv_out\.contiguous\(\)"):
        D.harris_detect_device(ctx, _Pyramid(), 4, 9, 40.0, torch.zeros(4, 3)[:, :2], torch.zeros(1, dtype=torch.int32))


def test_detect_device_of_the_detector_refuses_before_the_library(monkeypatch):
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    recorder = A.RecorderLib()
    monkeypatch.setattr(N, "lib", lambda: recorder)
    det = F.FeaturePointHarrisDetector(types.SimpleNamespace(handle=None))
    det.options().kMinFeatureDistance = 1
    points = torch.zeros(5, 2)
    for match, call in (("must not be negative", lambda: det.detect_device(_Pyramid(), -1)),
                        ("occupied_mask without occupied", lambda: det.detect_device(_Pyramid(), 4, None, torch.zeros(5, dtype=torch.uint8))),
                        ("^occupied must be a CUDA tensor", lambda: det.detect_device(_Pyramid(), 4, points)),
                        ("^occupied must be .*wrong dtype", lambda: det.detect_device(_Pyramid(), 4, points.double())),
                        ("^occupied must be .*dimension 1 is 3", lambda: det.detect_device(_Pyramid(), 4, torch.zeros(5, 3))),
                        (r"pass occupied\.contiguous\(\)", lambda: det.detect_device(_Pyramid(), 4, torch.zeros(5, 4)[:, ::2])),
                        ("FTK_HARRIS_DEVICE_MAX_SURVIVORS", lambda: det.detect_device(_Pyramid(257, 256), 4))):
        with pytest.raises(ValueError, match=match):
            call()
    assert recorder.calls == []


def test_video_tracker_refuses_bad_arguments_without_a_device(monkeypatch):
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    flow = F.OpticalFlowBasicKlt()
    for match, args, kwargs in (("flow must be", (None, 8), {}), ("flow must be", (F.OpticalFlow(), 8), {}), ("max_features must be in 1 .. 65536", (flow, 0), {}),
                                ("max_features must be in 1 .. 65536", (flow, 65537), {}), ("exceeds flow.options\\(\\).kMaxTrackPointsNumber = 500", (flow, 501), {}),
                                ("levels", (flow, 8), {"levels": 0}), ("levels", (flow, 8), {"levels": 13}), ("min_distance", (flow, 8), {"min_distance": 0}),
                                ("forward_backward", (flow, 8), {"forward_backward": -1.0}), ("forward_backward", (flow, 8), {"forward_backward": float("nan")}),
                                ("context_on_stream", (flow, 8), {"ctx": types.SimpleNamespace(handle=None)})):
        with pytest.raises(ValueError, match=match):
            F.KltVideoTracker(*args, **kwargs)
    recorder = A.RecorderLib()
    monkeypatch.setattr(N, "lib", lambda: recorder)
    tracker = F.KltVideoTracker(flow, 8, min_distance=1)
    assert tracker.ids is None and tracker.forward_backward is None and tracker.reset() is tracker
    good = np.zeros((40, 48), np.uint8)
    for match, bad in (("image must be", good.astype(np.float32)), ("image must be", good[None]), ("image must be", good.T), ("image must be", None),
                       ("image must be", torch.zeros(40, 48)), ("image must be", torch.zeros(1, 40, 48, dtype=torch.uint8)),
                       ("image must be contiguous", torch.zeros(48, 40, dtype=torch.uint8).t()), ("no CPU fallback", torch.zeros(40, 48, dtype=torch.uint8)),
                       ("at least 23 x 23", np.zeros((22, 48), np.uint8)), ("at least 23 x 23", np.zeros((40, 22), np.uint8)),
                       ("FTK_HARRIS_DEVICE_MAX_SURVIVORS", np.zeros((257, 256), np.uint8))):
        with pytest.raises(ValueError, match=match):
            tracker.track(bad)
    tracker._shape = (40, 48)  # as after a first frame
    with pytest.raises(ValueError, match=r"call reset\(\) before a sequence of another shape"):
        tracker.track(np.zeros((48, 40), np.uint8))
    flow.options().kMaxTrackPointsNumber = 4
    with pytest.raises(ValueError, match="kMaxTrackPointsNumber"):
        tracker.track(good)
    with pytest.raises(RuntimeError, match="before the first track"):
        tracker.live()
    assert recorder.calls == []


def test_header_library_and_binding_agree():
    from feature_tracker_amd import _native as N
    header = A.header_library_and_binding_agree(("FTK_HARRIS_DEVICE_MAX_SURVIVORS", "FTK_HARRIS_RANK_TILE", "FTK_TRACK_TABLE_MAX_SLOTS", "FTK_TRACK_TABLE_BLOCK"),
                                                {"ftk_harris_detect_device", "ftk_track_table_retire_device", "ftk_track_table_fill_device"})
    assert re.search(r"#define FTK_ABI_VERSION 1\b", header) and N.lib().ftk_abi_version() == 1
    lib = N.lib()  # null-context calls
    assert lib.ftk_harris_detect_device(None, None, 0, 0, 0, 0.0, None, None, 0, None, None) == -1
    assert lib.ftk_track_table_retire_device(None, 1, None, None, None, None, None, None, None, None, None, None, 0.0, None, None) == -1
    assert lib.ftk_track_table_fill_device(None, None, 0, 1, 0.0, 1, None, None, None, None, None, None, None, None, None) == -1


def test_nothing_in_the_package_imports_the_restatement():
    A.nothing_in_the_package_imports("track_table_ref")


def _plan(rows, cols, distance, slots, occupied):
    """The plan restated (csrc/track_table_plan.cpp)."""
    if rows < 1 or cols < 1 or occupied < 0 or rows * cols >= 1 << 32:
        return {"refused": "sizes"}
    if not 0 <= slots <= 65536:
        return {"refused": "slots"}
    d = max(distance, 1)
    bound = -(-rows // d) * -(-cols // d)
    centre = rows >= 23 and cols >= 23
    if centre and bound > 65536:
        return {"refused": "survivors"}
    capacity = bound if centre else 0
    return {"refused": "none", "distance": d, "reach": d - 1, "capacity": capacity, "image_blocks": -(-rows * cols // 256), "stamp_blocks": -(-occupied // 256),
            "rank_tile": 256, "rank_blocks": -(-capacity // 256), "rank_lds": 2048, "retire_block": 1024, "retire_per_thread": -(-slots // 1024),
            "retire_lds": 4096}


def test_plan_cli_equals_the_restated_plan():
    cases = []
    # survivor capacity 0, 1, tile, tile + 1, 65 536 (and one above); slots 1, 1 024, 1 025, 65 536 (and out of range)
    for rows, cols, d in ((22, 40, 3), (23, 23, 25), (32, 32, 2), (23, 6425, 25), (256, 256, 1), (257, 256, 1), (480, 752, 25), (480, 640, 8), (333, 251, 0),
                          (120, 160, -4), (0, 5, 1), (70000, 70000, 300)):
        for slots in (0, 1, 1024, 1025, 65536, 65537, -1):
            cases.append((rows, cols, d, slots, max(slots, 0)))
    cases.append((120, 160, 9, 8, -1))
    plans = A.run_plan_tool(PLAN_CLI, cases)
    seen = set()
    for case, got in zip(cases, plans):
        want = _plan(*case)
        assert got == {k: str(v) for k, v in want.items()}, (case, got, want)
        seen.add((want["refused"], want.get("capacity")))
    assert {("none", 0), ("none", 1), ("none", 256), ("none", 257), ("none", 65536), ("survivors", None), ("slots", None), ("sizes", None)} <= seen
