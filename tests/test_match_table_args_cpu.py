"""The loud failures of the landmark table and of ``MatchVideoTracker`` before any device is touched: the walk of
tests/args_walk.py over ``device.match_table_query_device`` and ``device.match_table_update_device``, their refusals, the refusals of
the library's own entries that need no device, the agreement of header, library and binding, and every ValueError of the class."""
import ctypes as C
import types

import pytest

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402


def _query(w, n=6, d=8):
    from feature_tracker_amd import device as D
    return D.match_table_query_device(w.ctx, w.t("ids", "int64", n), w.t("points", "float32", n, 2), w.t("descriptors", "float32", n, d),
                                      w.t("q_uv", "float32", n, 2), w.t("q_desc", "float32", n, d), w.t("q_slot", "int32", n), w.t("q_count", "int32", 1))


def _update(w, n=6, k=7, d=8, count=True, cur_slot=True, max_lost=1, words=None, alias=None):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    t = dict(ids=w.t("ids", "int64", n), points=w.t("points", "float32", n, 2), prev_points=w.t("prev_points", "float32", n, 2),
             descriptors=w.t("descriptors", "float32", n, d), status=w.t("status", "uint8", n), age=w.t("age", "int32", n), lost=w.t("lost", "int32", n),
             n_live=w.t("n_live", "int32", 1), next_id=w.t("next_id", "int64", 1), q_slot=w.t("q_slot", "int32", n), q_count=w.t("q_count", "int32", 1),
             match_index=w.t("match_index", "int32", n), match_status=w.t("match_status", "uint8", n), cur_uv=w.t("cur_uv", "float32", k, 2),
             cur_desc=w.t("cur_desc", "float32", k, d))
    t["cur_count"] = w.t("cur_count", "int32", 1) if count else None
    need = -(-N.match_table_workspace_bytes(n, k, d) // 8)
    t["workspace"] = w.t("workspace", "int64", need if words is None else words)
    t["cur_slot"] = w.t("cur_slot", "int32", k) if cur_slot else None
    if alias:
        t[alias[0]] = t[alias[1]]
    return D.match_table_update_device(w.ctx, *[t[name] for name in ("ids", "points", "prev_points", "descriptors", "status", "age", "lost", "n_live", "next_id",
                                                                       "q_slot", "q_count", "match_index", "match_status", "cur_uv", "cur_desc", "cur_count")],
                                       max_lost, t["workspace"], t["cur_slot"])


def test_entries_take_no_pointer_of_an_unchecked_argument(monkeypatch):
    A.walk_call(monkeypatch, _query, ["ftk_match_table_query_device"])
    for kw in (dict(), dict(count=False), dict(cur_slot=False), dict(n=1, k=1, d=1), dict(n=4096, k=4096, d=1024)):
        A.walk_call(monkeypatch, lambda w: _update(w, **kw), ["ftk_match_table_update_device"])


@pytest.mark.parametrize("kind", ["dtype", "shape", "device"])
def test_each_refused_tensor_stops_the_entries_before_the_library(monkeypatch, kind):
    def reshape(fake):  # (a row fewer of the tensor that sizes the call is a valid tensor: a column fewer is not)
        return (fake.shape[0], fake.shape[1] - 1) if fake.name in ("descriptors", "cur_uv") else A.one_row_fewer(fake)

    # (ids, descriptors and cur_uv size the call: spoiled in shape, a tensor sized by them is the one refused)
    A.refusal_sweep(monkeypatch, _query, kind, loose=("ids", "descriptors"), reshape=reshape)
    names = A.refusal_sweep(monkeypatch, _update, kind, loose=("ids", "descriptors", "cur_uv"), reshape=reshape)
    assert len(names) == 18


def test_other_refusals(monkeypatch):
    w = A.Walk(monkeypatch)
    for match, kw in (("FTK_MATCH_TABLE_MAX_SLOTS", dict(n=4097)), ("FTK_MATCH_TABLE_MAX_SLOTS", dict(n=0)), ("FTK_MATCH_TABLE_MAX_SLOTS", dict(k=4097)),
                      ("FTK_MATCH_TABLE_MAX_SLOTS", dict(k=0)), ("FTK_MATCH_TABLE_MAX_DIM", dict(d=1025)), ("FTK_MATCH_TABLE_MAX_DIM", dict(d=0)),
                      ("max_lost must be an integer >= 0", dict(max_lost=-1)), ("max_lost must be", dict(max_lost=1.0)), ("max_lost must be", dict(max_lost=True)),
                      ("max_lost must be", dict(max_lost=None)), ("^workspace must be .*too few", dict(words=3)),
                      ("cur_slot and q_slot are one tensor", dict(alias=("cur_slot", "q_slot"))), ("no argument may alias another", dict(alias=("prev_points", "points"))),
                      ("no argument may alias another", dict(alias=("cur_desc", "descriptors")))):
        with pytest.raises(ValueError, match=match):
            _update(w, **kw)
    for match, kw in (("FTK_MATCH_TABLE_MAX_SLOTS", dict(n=4097)), ("FTK_MATCH_TABLE_MAX_SLOTS", dict(n=0)), ("FTK_MATCH_TABLE_MAX_DIM", dict(d=1025))):
        with pytest.raises(ValueError, match=match):
            _query(w, **kw)
    from feature_tracker_amd import device as D
    one = w.t("one", "float32", 6, 2)
    with pytest.raises(ValueError, match="q_uv and points are one tensor"):
        D.match_table_query_device(w.ctx, w.t("ids", "int64", 6), one, w.t("descriptors", "float32", 6, 8), one, w.t("q_desc", "float32", 6, 8),
                                   w.t("q_slot", "int32", 6), w.t("q_count", "int32", 1))
    assert w.lib.calls == [] and w.unchecked_reads == []


def test_header_library_and_binding_agree():
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    header = A.header_library_and_binding_agree(("FTK_MATCH_TABLE_MAX_SLOTS", "FTK_MATCH_TABLE_MAX_DIM"),
                                                {"ftk_match_table_workspace_bytes", "ftk_match_table_query_device", "ftk_match_table_update_device"})
    assert "nn_feature_matcher.cpp:187-215" in header
    assert N.FTK_MATCH_TABLE_MAX_SLOTS == N.FTK_TRANSFORMER_MAX_ROWS == N.FTK_MATCH_ASSIGNMENT_MAX_ROWS == 4 * N.FTK_TRACK_TABLE_BLOCK
    assert "MatchVideoTracker" in F.__all__ and callable(D.match_table_query_device) and callable(D.match_table_update_device)
    lib, out = N.lib(), C.c_int64()
    for n in (1, 63, 1025, 4096):
        for k in (1, 3, 4, 5, 1023, 4096):
            for d in (1, 256, 1024):
                assert lib.ftk_match_table_workspace_bytes(n, k, d, C.byref(out)) == 0
                assert out.value == N.match_table_workspace_bytes(n, k, d) and out.value % 16 == 0 and out.value >= 4 * k
    bytes_of = lib.ftk_match_table_workspace_bytes
    assert bytes_of(0, 1, 1, C.byref(out)) == -1 and bytes_of(4097, 1, 1, C.byref(out)) == -1 and bytes_of(1, 0, 1, C.byref(out)) == -1
    assert bytes_of(1, 4097, 1, C.byref(out)) == -1 and bytes_of(1, 1, 0, C.byref(out)) == -1 and bytes_of(1, 1, 1025, C.byref(out)) == -1
    assert bytes_of(1, 1, 1, None) == -1
    assert lib.ftk_match_table_query_device(None, None, 1, 1, *[None] * 7) == -1  # null context
    assert lib.ftk_match_table_update_device(None, None, 1, 1, *[None] * 15, 1, None, 0, None, None) == -1


def test_nothing_in_the_package_imports_the_restatement():
    A.nothing_in_the_package_imports("match_table_ref")
    A.nothing_in_the_package_imports("match_video_cases")


def _lightglue(d=32, heads=2, layers=2, adaptive=False, seed=0):
    from tests import match_video_weights as W
    import feature_tracker_amd as F
    kw = dict(depth_confidence=0.95, width_confidence=0.99) if adaptive else {}
    return F.LightGlue.from_state_dict(W.lightglue_state(d, heads, layers, seed), num_heads=heads, **kw)


def test_every_value_error_of_the_class(monkeypatch):
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    from tests import match_video_weights as W
    recorder = A.RecorderLib()
    monkeypatch.setattr(N, "lib", lambda: recorder)
    head = F.MatchAssignment.without_weights(16)
    lg = _lightglue()
    sp = F.SuperPoint.from_state_dict(W.superpoint_state(32, 0))
    dec = F.KeypointDecoder(max_keypoints=40)
    T = F.MatchVideoTracker
    for match, make in (("matcher must be a LightGlue or a MatchAssignment", lambda: T(object(), 8)),
                        ("max_tracks must be an integer in 1", lambda: T(head, 0)), ("max_tracks must be", lambda: T(head, 4097)),
                        ("max_tracks must be", lambda: T(head, 8.0)), ("max_tracks must be", lambda: T(head, True)),
                        ("max_lost must be an integer >= 0", lambda: T(head, 8, max_lost=-1)), ("max_lost must be", lambda: T(head, 8, max_lost=0.5)),
                        ("min_score must be a number", lambda: T(head, 8, min_score=float("nan"))), ("min_score must be", lambda: T(head, 8, min_score="low")),
                        ("adaptive=True needs a LightGlue", lambda: T(head, 8, adaptive=True)),
                        ("adaptive=True needs LightGlue.from_state_dict", lambda: T(lg, 8, adaptive=True)),
                        ("detector must be \\(SuperPoint, KeypointDecoder\\)", lambda: T(lg, 8, detector=sp)),
                        ("detector must be", lambda: T(lg, 8, detector=(dec, sp))),
                        ("the detector's descriptors have 32 channels, the matcher takes 16", lambda: T(head, 8, detector=(sp, dec))),
                        ("max_keypoints 5000 exceeds", lambda: T(lg, 8, detector=(sp, F.KeypointDecoder(max_keypoints=5000)))),
                        ("geometric must be a TwoViewRansac or an EpipolarRansac", lambda: T(head, 8, geometric="homography")),
                        ("geometric_seed must be a uint32", lambda: T(head, 8, geometric_seed=-1)),
                        ("geometric_seed must be", lambda: T(head, 8, geometric_seed=1 << 32)),
                        ("context_on_stream", lambda: T(head, 8, ctx=types.SimpleNamespace(handle=None)))):
        with pytest.raises(ValueError, match=match):
            make()
    assert T(lg, 8, adaptive=False).dim == 32 and T(_lightglue(adaptive=True), 4096, adaptive=True, max_lost=3).max_lost == 3
    uv, desc, one = torch.zeros(7, 2), torch.zeros(7, 16), torch.zeros(1, dtype=torch.int32)
    plain, filtered, learned = T(head, 8), T(head, 8, geometric=F.TwoViewRansac("homography")), T(lg, 8)
    for match, tracker, args, kw in (("^uv must be .*wrong dtype", plain, (uv.double(), desc), {}), ("^uv must be .*dimension 1 is 3", plain, (torch.zeros(7, 3), desc), {}),
                                     ("^descriptors must be .*dimension 1 is 15", plain, (uv, torch.zeros(7, 15)), {}),
                                     ("^descriptors must be .*dimension 0 is 6", plain, (uv, torch.zeros(6, 16)), {}),
                                     ("^descriptors must be .*strided view", plain, (uv, torch.zeros(7, 32)[:, ::2]), {}),
                                     ("^uv must be a torch tensor", plain, (None, desc), {}),
                                     ("FTK_MATCH_TABLE_MAX_SLOTS", plain, (torch.zeros(4097, 2), torch.zeros(4097, 16)), {}),
                                     ("FTK_MATCH_TABLE_MAX_SLOTS", plain, (torch.zeros(0, 2), torch.zeros(0, 16)), {}),
                                     ("^count must be .*wrong dtype", plain, (uv, desc, one.long()), {}), ("^count must be .*dimension 0 is 2", plain, (uv, desc, torch.zeros(2, dtype=torch.int32)), {}),
                                     ("image_size=\\(W, H\\) is required with a LightGlue", learned, (uv, torch.zeros(7, 32)), {}),
                                     ("image_size=\\(W, H\\) is required with a geometric filter", filtered, (uv, desc), {}),
                                     ("image_size must be \\(width, height\\)", plain, (uv, desc), dict(image_size=(0, 5))),
                                     ("image_size must be", learned, (uv, torch.zeros(7, 32)), dict(image_size=128)),
                                     ("image_size must be \\(H, W\\) with both in 1 .. 65536", filtered, (uv, desc), dict(image_size=(70000, 5))),
                                     ("^descriptors must be .*dimension 1 is 16", learned, (uv, desc), dict(image_size=(128, 96))),
                                     ("no CPU fallback", plain, (uv, desc), {}), ("no CPU fallback", plain, (uv, desc, one), dict(image_size=(128, 96)))):
        with pytest.raises(ValueError, match=match):
            tracker.update(*args, **kw)
    with pytest.raises(ValueError, match="track\\(image\\) needs detector"):
        plain.track(torch.zeros(96, 128))
    with pytest.raises(ValueError, match="image must be a float32 CUDA tensor"):
        T(lg, 8, detector=(sp, dec)).track(torch.zeros(96, 128, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="before the first update"):
        plain.live()
    assert plain.reset() is plain and plain.ids is None
    assert recorder.calls == []
