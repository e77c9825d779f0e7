"""The loud failures of the warm start's entries, of ``flow_init`` and of ``RaftVideoTracker`` before any device is touched (DESIGN.md
5.18): what tests/test_flow_warm_gpu.py and tests/test_raft_video_gpu.py check on a device, as far as it can be checked without one;
the walk of tests/args_walk.py (duck-typed tensors, a recording stand-in for the native library) over
``device.flow_warm_device``; and the agreement of header, library and binding."""
import re
import types

import pytest

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402


def test_warm_start_flow_refuses_bad_arguments_without_a_device():
    import feature_tracker_amd as F
    flow = torch.zeros(2, 2, 3, 5)
    for match, bad in (("flow must be", flow.double()), ("flow must be", flow.half()), ("flow must be", flow[0]), ("flow must be", torch.zeros(2, 3, 3, 5)),
                       ("flow must be", flow.numpy()), ("flow must be", None), ("must not be empty", torch.zeros(2, 2, 0, 5)),
                       ("must not be empty", torch.zeros(0, 2, 3, 5)), ("FTK_FLOW_WARM_MAX_PIXELS", torch.zeros(1, 2, 1025, 1024)),
                       ("contiguous", torch.zeros(2, 2, 5, 3).transpose(2, 3)), ("contiguous", torch.zeros(2, 4, 3, 5)[:, ::2]),
                       ("no CPU fallback", flow)):
        with pytest.raises(ValueError, match=match):
            F.warm_start_flow(bad)
    with pytest.raises(RuntimeError, match="warm_start_flow is inference only"):
        F.warm_start_flow(flow.clone().requires_grad_(True))


def test_device_entry_refuses_bad_arguments_without_a_device():
    from feature_tracker_amd import device as D
    ctx = types.SimpleNamespace(handle=None)
    flow, out = torch.zeros(1, 2, 3, 5), torch.zeros(1, 2, 3, 5)
    with pytest.raises(ValueError, match="^flow must be a CUDA tensor"):
        D.flow_warm_device(ctx, flow, out)
    with pytest.raises(ValueError, match="^flow must be .*wrong dtype"):
        D.flow_warm_device(ctx, flow.double(), out)
    for splits in (0, -1, 33):
        with pytest.raises(ValueError, match="splits must be in 1 .. 32"):
            D.flow_warm_device(ctx, flow, out, splits, torch.zeros(1000, dtype=torch.int64))
    with pytest.raises(ValueError, match="go together"):
        D.flow_warm_device(ctx, flow, out, 2)
    with pytest.raises(ValueError, match="go together"):
        D.flow_warm_device(ctx, flow, out, 1, torch.zeros(1000, dtype=torch.int64))


def _walk_call(w, splits=3, words=3 * 2 * 3 * 5):
    from feature_tracker_amd import device as D
    return D.flow_warm_device(w.ctx, w.t("flow", "float32", 2, 2, 3, 5), w.t("out", "float32", 2, 2, 3, 5), splits, w.t("workspace", "int64", words))


def test_device_entry_takes_no_pointer_of_an_unchecked_argument(monkeypatch):
    from feature_tracker_amd import device as D
    A.walk_call(monkeypatch, _walk_call, ["ftk_flow_warm_device"])
    one_split = lambda w: D.flow_warm_device(w.ctx, w.t("flow", "float32", 2, 2, 3, 5), w.t("out", "float32", 2, 2, 3, 5))  # noqa: E731  (no workspace)
    A.walk_call(monkeypatch, one_split, ["ftk_flow_warm_device"])


@pytest.mark.parametrize("which,change,match", [
    (0, ("dtype", "int32"), "flow must be"), (1, ("dtype", "int32"), "out must be"), (2, ("dtype", "float32"), "workspace must be"),
    (0, ("shape", (2, 3, 3, 5)), "flow must be.*dimension 1 is 3, not 2"), (0, ("shape", (2, 2, 15)), "flow must be.*3 dimensions instead of 4"),
    (0, ("shape", (2, 2, 0, 5)), "non-empty"), (0, ("shape", (1, 2, 1025, 1024)), "FTK_FLOW_WARM_MAX_PIXELS"),
    (1, ("shape", (2, 2, 5, 3)), "out must be.*dimension 2 is 5, not 3"), (1, ("shape", (1, 2, 3, 5)), "out must be.*dimension 0"),
    (2, ("shape", (89,)), "workspace must be.*89 elements are too few"), (2, ("shape", (45, 2)), "workspace must be.*2 dimensions instead of 1"),
    (1, ("device", 1), "out must be on cuda:0"), (2, ("device", 1), "workspace must be on cuda:0"),
])
def test_device_entry_stops_before_the_library(monkeypatch, which, change, match):
    A.refused_call(monkeypatch, _walk_call, (which, *change), match)


def test_header_library_and_binding_agree():
    from feature_tracker_amd import _native as N
    header = A.header_library_and_binding_agree(("FTK_FLOW_WARM_TILE", "FTK_FLOW_WARM_MAX_SPLITS"), {"ftk_flow_warm_splits", "ftk_flow_warm_device"})
    assert re.search(r"#define FTK_FLOW_WARM_MAX_PIXELS \(1 << (\d+)\)", header).group(1) == "20" and N.FTK_FLOW_WARM_MAX_PIXELS == 1 << 20


def test_split_rule_and_native_refusals_need_no_device():
    """ftk_flow_warm_splits: 1 where the targets alone fill the chip or there is one tile of sources, never more splits than tiles of
    sources or than the maximum; the refusals of both native entries come before anything touches a device."""
    from feature_tracker_amd import _native as N
    T = N.FTK_FLOW_WARM_TILE
    for B, H, W in ((1, 1, 1), (1, 8, 8), (3, 16, 16), (1, 33, 65), (3, 33, 65), (1, 55, 128), (5, 55, 128), (1, 135, 240), (1, 1024, 1024), (4096, 16, 16)):
        tiles = -(-H * W // T)
        want = min(-(-1024 // (tiles * B)), tiles, N.FTK_FLOW_WARM_MAX_SPLITS)
        assert N.flow_warm_splits(B, H, W) == want, (B, H, W)
    assert N.flow_warm_splits(1, 33, 65) >= 2 and N.flow_warm_splits(3, 33, 65) >= 2  # what tests/test_flow_warm_gpu.py counts on
    for bad in ((0, 3, 5), (1, 0, 5), (1, 3, -1), (1, 1025, 1024)):
        with pytest.raises(N.FtkError, match="FTK_E_INVALID_ARGUMENT"):
            N.flow_warm_splits(*bad)
    assert N.lib().ftk_flow_warm_splits(1, 3, 5, None) == -1
    assert N.lib().ftk_flow_warm_device(None, None, None, 1, 3, 5, 1, None, None) == -1  # null context


def test_raft_flow_init_refused_without_a_device(monkeypatch):
    """The checks of ``flow_init`` in Raft.__call__ and Raft.track_points, every one before the first launch: the recording library sees
    none."""
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    from tests.test_raft_encoder_cpu import RAFT_CASES, make_image, make_raft_state
    c = RAFT_CASES[0]
    model = F.Raft.from_state_dict(make_raft_state(c, 1), c[3], c[4], max_iterations=2)
    recorder = A.RecorderLib()
    monkeypatch.setattr(N, "lib", lambda: recorder)
    ref, cur, pts = make_image(1, 1, 16, 24, 1), make_image(1, 1, 16, 24, 2), torch.zeros(1, 5, 2)
    good = torch.zeros(1, 2, 2, 3)  # 16 x 24 images give 2 x 3 feature maps
    for bad in (good.double(), good[0], torch.zeros(1, 2, 3, 2), torch.zeros(2, 2, 2, 3), torch.zeros(1, 3, 2, 3), good.numpy(), (good, good)):
        with pytest.raises(ValueError, match="flow_init must be"):
            model(ref, cur, flow_init=bad)
        with pytest.raises(ValueError, match="flow_init must be"):
            model.track_points(ref, cur, pts, flow_init=bad)
    for bad in (good, (good,), (good, good, good)):
        with pytest.raises(ValueError, match="flow_init must be a \\(forward_init, backward_init\\) pair"):
            model.track_points(ref, cur, pts, forward_backward=1.0, flow_init=bad)
    with pytest.raises(ValueError, match="flow_init\\[1\\] must be"):
        model.track_points(ref, cur, pts, forward_backward=1.0, flow_init=(good, good.double()))
    with pytest.raises(RuntimeError, match="Raft is inference only"):
        model(ref, cur, flow_init=good.clone().requires_grad_(True))
    for call in (lambda: model(ref, cur, flow_init=good, return_flow=True), lambda: model.track_points(ref, cur, pts, flow_init=good, return_flow=True),
                 lambda: model.track_points(ref, cur, pts, forward_backward=1.0, flow_init=(good, good))):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    assert recorder.calls == []


def test_video_tracker_refuses_bad_arguments_without_a_device(monkeypatch):
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    from tests.test_raft_encoder_cpu import RAFT_CASES, make_image, make_raft_state
    c = RAFT_CASES[0]
    model = F.Raft.from_state_dict(make_raft_state(c, 1), c[3], c[4], max_iterations=2)
    for match, args, kwargs in (("raft must be a Raft", (None,), {}), ("iterations 0", (model,), {"iterations": 0}),
                                ("forward_backward", (model,), {"forward_backward": -1.0}), ("forward_backward", (model,), {"forward_backward": float("nan")})):
        with pytest.raises(ValueError, match=match):
            F.RaftVideoTracker(*args, **kwargs)
    recorder = A.RecorderLib()
    monkeypatch.setattr(N, "lib", lambda: recorder)
    tracker = F.RaftVideoTracker(model)
    assert tracker.last_flow is None and tracker.iterations == 2 and tracker.warm_start and tracker.forward_backward is None
    image = make_image(1, 1, 16, 24, 1)
    for match, bad in (("image must be", image.double()), ("image must be", image[0]), ("image must be", None), ("no CPU fallback", image)):
        with pytest.raises(ValueError, match=match):
            tracker.track(bad)
    assert recorder.calls == [] and tracker.last_flow is None
