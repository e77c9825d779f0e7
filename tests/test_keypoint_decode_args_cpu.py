"""The loud failures of the keypoint decoder before any device is touched: the walk of tests/args_walk.py over
``device.keypoint_decode_device``; the refusals of ``KeypointDecoder``; the agreement of header, library and binding; and the launch plan
through host/build/keypoint_decode_plan_cli."""
import types

import pytest

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402

PLAN_CLI = A.plan_cli("keypoint_decode_plan_cli")


def _call(w, hc=3, wc=5, d=16, k=10, min_score=0.1, min_distance=4, border=4, n_occ=6, layout="chw", mask=True, heatmap=True):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    semi = w.t("semi", "float32", 65, hc, wc)
    desc = w.t("desc", "float32", d, hc, wc) if layout == "chw" else w.t("desc", "float32", hc, wc, d)
    occupied = w.t("occupied", "float32", n_occ, 2) if n_occ else None
    occupied_mask = w.t("occupied_mask", "uint8", n_occ) if n_occ and mask else None
    words = -(-N.keypoint_decode_workspace_bytes(min(max(hc, 1), 8192), min(max(wc, 1), 8192), min_distance if isinstance(min_distance, int) else 1, n_occ) // 8)
    return D.keypoint_decode_device(w.ctx, semi, desc, k, min_score, min_distance, border, w.t("workspace", "int64", words), w.t("uv", "float32", k, 2),
                                    w.t("scores", "float32", k), w.t("descriptors", "float32", k, d), w.t("count", "int32", 1),
                                    w.t("heatmap", "float32", 8 * hc, 8 * wc) if heatmap else None, occupied, occupied_mask, layout)


def test_entry_takes_no_pointer_of_an_unchecked_argument(monkeypatch):
    for layout in ("chw", "hwc"):
        A.walk_call(monkeypatch, lambda w: _call(w, layout=layout), ["ftk_keypoint_decode_device"])


@pytest.mark.parametrize("kind", ["dtype", "shape", "device"])
def test_each_refused_tensor_stops_the_entry_before_the_library(monkeypatch, kind):
    # (one channel or one occupied point fewer is a valid tensor: the next tensor sized by it is the one refused)
    A.refusal_sweep(monkeypatch, _call, kind, loose=("desc", "occupied", "workspace"))


def test_other_refusals(monkeypatch):
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    w = A.Walk(monkeypatch)
    for match, kw in (("max_keypoints must be in 1 .. FTK_KEYPOINT_DECODE_MAX_KEYPOINTS", dict(k=0)), ("max_keypoints must be in", dict(k=65537)),
                      ("min_score must be a finite", dict(min_score=float("nan"))), ("min_score must be a finite", dict(min_score=float("inf"))),
                      ("min_score must be a finite", dict(min_score="high")), ("border must not be negative", dict(border=-1)),
                      ("min_distance must be an integer", dict(min_distance=2.5)), ("border must be an integer", dict(border=True)),
                      ("FTK_HARRIS_DEVICE_MAX_SURVIVORS", dict(hc=64, wc=64, min_distance=1)), ("FTK_KEYPOINT_DECODE_MAX_CHANNELS", dict(d=1025)),
                      ("at most 65536 x 65536", dict(hc=8193, wc=1, min_distance=4096)), ("desc_layout must be one of", dict(layout="nhwc"))):
        with pytest.raises(ValueError, match=match):
            _call(w, **kw)
    with pytest.raises(ValueError, match="occupied_mask without occupied"):
        from feature_tracker_amd import device as D
        D.keypoint_decode_device(w.ctx, None, None, 4, 0.1, 4, 4, None, None, None, None, None, occupied_mask=w.t("occupied_mask", "uint8", 3))
    assert w.lib.calls == [] and w.unchecked_reads == []
    for kw in (dict(), dict(n_occ=0), dict(mask=False), dict(heatmap=False), dict(layout="hwc"), dict(d=1), dict(d=1024), dict(min_distance=0), dict(min_distance=-3),
               dict(hc=1, wc=1, border=0), dict(hc=32, wc=32, min_distance=1)):
        _call(w, **kw)
    assert len(w.lib.calls) == 11
    recorder = A.RecorderLib()
    monkeypatch.setattr(N, "lib", lambda: recorder)
    for match, kw in (("max_keypoints", dict(max_keypoints=0)), ("max_keypoints", dict(max_keypoints=1.5)), ("min_score", dict(min_score=float("nan"))),
                      ("min_distance", dict(min_distance="far")), ("border", dict(border=-4)), ("context_on_stream", dict(ctx=types.SimpleNamespace(handle=None)))):
        with pytest.raises(ValueError, match=match):
            F.KeypointDecoder(**kw)
    decoder = F.KeypointDecoder()
    # the reference's NNFeaturePointDetector::Options, and upstream SuperPoint's border
    assert (decoder.max_keypoints, decoder.min_score, decoder.min_distance, decoder.border) == (300, 0.1, 20, 4)
    semi, desc = torch.zeros(65, 3, 5), torch.zeros(16, 3, 5)
    for match, args, kw in (("^semi must be .*wrong dtype", (semi.double(), desc), {}), ("^semi must be .*dimension 0 is 64", (semi[:64], desc), {}),
                            ("^desc must be .*wrong dtype", (semi, desc.double()), {}), ("^desc must be .*dimension 2 is 4", (semi, torch.zeros(16, 3, 4)), {}),
                            ("^desc must be a float32 tensor of shape", (semi, torch.zeros(16, 15)), {}),
                            ("^desc must be a contiguous .* or a permute", (semi, torch.zeros(16, 3, 10)[:, :, ::2]), {}),
                            ("^occupied must be .*dimension 1 is 3", (semi, desc), dict(occupied=torch.zeros(4, 3))),
                            ("occupied_mask without occupied", (semi, desc), dict(occupied_mask=torch.zeros(4, dtype=torch.uint8))),
                            ("no CPU fallback", (semi, desc), {}), ("no CPU fallback", (semi, torch.zeros(3, 5, 16).permute(2, 0, 1)), {})):
        with pytest.raises(ValueError, match=match):
            decoder.decode(*args, **kw)
    with pytest.raises(ValueError, match="FTK_HARRIS_DEVICE_MAX_SURVIVORS"):
        F.KeypointDecoder(min_distance=1).decode(torch.zeros(65, 64, 64), torch.zeros(4, 64, 64))
    assert recorder.calls == []


def test_header_library_and_binding_agree():
    import ctypes as C
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    A.header_library_and_binding_agree(("FTK_KEYPOINT_DECODE_CELL", "FTK_KEYPOINT_DECODE_MAX_KEYPOINTS", "FTK_KEYPOINT_DECODE_MAX_CHANNELS"),
                                       {"ftk_keypoint_decode_workspace_bytes", "ftk_keypoint_decode_device"})
    assert {"KeypointDecoder", "KeypointResult"} <= set(F.__all__) and callable(D.keypoint_decode_device)
    lib, out = N.lib(), C.c_int64()
    for hc, wc in ((1, 1), (3, 5), (2, 65), (9, 17), (60, 94), (60, 80)):
        for distance in (-1, 0, 1, 4, 9, 20):
            for n_occ in (0, 1, 300):
                if -(-8 * hc // max(distance, 1)) * -(-8 * wc // max(distance, 1)) > N.FTK_HARRIS_DEVICE_MAX_SURVIVORS:
                    assert lib.ftk_keypoint_decode_workspace_bytes(hc, wc, distance, n_occ, C.byref(out)) == -4  # FTK_E_UNSUPPORTED
                    continue
                assert lib.ftk_keypoint_decode_workspace_bytes(hc, wc, distance, n_occ, C.byref(out)) == 0
                assert out.value == N.keypoint_decode_workspace_bytes(hc, wc, distance, n_occ) and out.value % 16 == 0
    assert lib.ftk_keypoint_decode_workspace_bytes(0, 1, 4, 0, C.byref(out)) == -1 and lib.ftk_keypoint_decode_workspace_bytes(1, 8193, 4096, 0, C.byref(out)) == -1
    assert lib.ftk_keypoint_decode_workspace_bytes(1, 1, 4, -1, C.byref(out)) == -1 and lib.ftk_keypoint_decode_workspace_bytes(1, 1, 4, 0, None) == -1
    assert lib.ftk_keypoint_decode_device(None, None, None, 1, 1, None, 1, 1, 1, 1, 1, 0.1, 1, 0, None, None, 0, None, None, None, None, None, None) == -1  # null context


def test_nothing_in_the_package_imports_the_restatement():
    A.nothing_in_the_package_imports("keypoint_decode_ref")


def _plan(hc, wc, d, k, distance, border, n_occ):
    """The plan restated (csrc/keypoint_decode_plan.cpp)."""
    if not (1 <= hc <= 8192 and 1 <= wc <= 8192) or border < 0 or n_occ < 0:
        return {"refused": "sizes"}
    if not 1 <= d <= 1024:
        return {"refused": "channels"}
    if not 1 <= k <= 65536:
        return {"refused": "keypoints"}
    rows, cols, dist = 8 * hc, 8 * wc, max(distance, 1)
    capacity = -(-rows // dist) * -(-cols // dist)
    if capacity > 65536:
        return {"refused": "survivors"}
    up16 = lambda v: (v + 15) & ~15  # noqa: E731
    px = rows * cols
    off_tmp = up16(8 * px)
    off_wmax = off_tmp + up16(8 * px)
    off_list = off_wmax + up16(8 * px)
    off_count = off_list + up16(8 * capacity)
    off_plane = off_count + 16
    off_dilated = off_plane + (up16(px) if n_occ else 0)
    return {"refused": "none", "rows": rows, "cols": cols, "distance": dist, "reach": dist - 1, "capacity": capacity, "score_tile": 64,
            "score_grid_x": -(-wc // 64), "score_grid_y": hc, "score_lds": 64 * 68 * 4, "image_blocks": -(-px // 256), "stamp_blocks": -(-n_occ // 256),
            "rank_tile": 256, "rank_blocks": -(-capacity // 256), "describe_waves": 4, "describe_blocks": -(-k // 4), "launches": 10 if n_occ else 7,
            "memsets": 4 if n_occ else 3, "off_tmp": off_tmp, "off_wmax": off_wmax, "off_list": off_list, "off_count": off_count, "off_plane": off_plane,
            "off_dilated": off_dilated, "bytes": off_dilated + (up16(px) if n_occ else 0)}


def test_plan_cli_equals_the_restated_plan():
    from feature_tracker_amd import _native as N
    cases = [(hc, wc, d, k, distance, 4, n_occ) for hc, wc in ((1, 1), (3, 5), (2, 65), (9, 17), (60, 94), (60, 80), (8192, 8192), (0, 5), (3, 8193), (-1, -1))
             for d, k in ((1, 1), (64, 300), (65, 3), (256, 2000), (1024, 65536), (0, 300), (1025, 300), (256, 0), (256, 65537))
             for distance in (-2, 0, 1, 4, 9, 20, 256) for n_occ in (0, 1, 256, 257)]
    cases += [(3, 5, 64, 300, 4, -1, 0), (3, 5, 64, 300, 4, 0, -1), (3, 5, 64, 300, 4, 1000, 0)]
    plans = A.run_plan_tool(PLAN_CLI, cases)
    seen = set()
    for case, got in zip(cases, plans):
        want = _plan(*case)
        assert got == {k: str(v) for k, v in want.items()}, (case, got, want)
        seen.add(want["refused"])
        if want["refused"] == "none":
            assert want["bytes"] == N.keypoint_decode_workspace_bytes(case[0], case[1], case[4], case[6])
            assert want["score_lds"] <= 65536 and want["score_grid_y"] <= 65535
    assert seen == {"none", "sizes", "survivors", "keypoints", "channels"}
