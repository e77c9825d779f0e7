"""``flow_init`` / ``return_flow`` of Raft and RaftVideoTracker on the device, at the model and images of
tests/test_raft_points_gpu.py: a zero ``flow_init`` changes no bit; a Gaussian one gives the loop written out here from the public parts,
started from ``ref + flow_init``; a tracker without the warm start equals pairwise ``track_points`` bit for bit (the cached feature map
is the half of the stacked call's); a tracker with it equals ``track_points`` started from ``warm_start_flow`` of the previous pair's
flow, with and without the forward-backward check, and differs from the cold result; ``reset()``, ``points=None``, a frame of another
shape; and the count of library entries per frame."""
import functools

import numpy as np
import pytest

from tests import flow_points_ref as P
from tests.test_flow_points_cpu import point_set
from tests.test_raft_encoder_cpu import make_image
from tests.test_raft_points_gpu import B, COUNT, ITERATIONS, SIZES, models, on_device

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = ["all_pairs", "on_demand"]
IDS = ["60x60", "44x68"]


def grid(size):
    return tuple((((e + 1) // 2 + 1) // 2 + 1) // 2 for e in size)


@functools.lru_cache(maxsize=None)
def frames(size):
    """(f0, f1, f2 on the device, points on the device): three seeds, computed once, never written to."""
    H, W = size
    h, w = grid(size)
    return tuple(on_device(make_image(B, 1, H, W, 60 + k)) for k in range(3)), on_device(point_set(B, h, w, COUNT, size, 17))


def host(result):
    return [None if r is None else r.cpu().numpy() for r in result]


def equal(got, want):
    got, want = host(got), host(want)
    return len(got) == len(want) and all((g is None and w is None) or (g is not None and w is not None and P.same(g, w)) for g, w in zip(got, want))


def gaussian_init(size, seed, batch=B):
    h, w = grid(size)
    return on_device((np.random.default_rng(seed).standard_normal((batch, 2, h, w)) * 1.5).astype(np.float32))


@functools.lru_cache(maxsize=None)
def threshold(ftk, mode, size):
    """A forward-backward threshold that separates the points, chosen as tests/test_raft_points_gpu.py chooses it: the median
    forward-backward distance of the pair (f0, f1)."""
    (f0, f1, _), points = frames(size)
    _, _, e2 = models(ftk)[mode].track_points(f0, f1, points, forward_backward=1e18, return_error=True)  # every point that comes back passes
    e2 = e2.cpu().numpy()
    return float(np.sqrt(np.median(e2[e2 > 0])))


@pytest.mark.parametrize("size", SIZES, ids=IDS)
@pytest.mark.parametrize("mode", MODES)
def test_a_zero_flow_init_changes_no_bit(ftk, mode, size):
    model = models(ftk)[mode]
    (f0, f1, _), points = frames(size)
    h, w = grid(size)
    zeros = torch.zeros(B, 2, h, w, device="cuda")
    plain = model(f0, f1)
    assert isinstance(plain, list) and len(plain) == ITERATIONS
    assert equal(model(f0, f1, flow_init=zeros), plain)
    assert equal(model.track_points(f0, f1, points, flow_init=zeros), model.track_points(f0, f1, points))
    t = threshold(ftk, mode, size)
    assert equal(model.track_points(f0, f1, points, forward_backward=t, return_error=True, flow_init=(zeros, zeros)),
                 model.track_points(f0, f1, points, forward_backward=t, return_error=True))
    predictions, flow = model(f0, f1, return_flow=True)
    assert equal(predictions, plain) and flow.shape == (B, 2, h, w)
    cur, status, flow_again = model.track_points(f0, f1, points, return_flow=True)
    assert P.same(flow_again.cpu().numpy(), flow.cpu().numpy())  # the two loops differ by the mask head alone
    assert equal((cur, status), model.track_points(f0, f1, points))


@pytest.mark.parametrize("size", SIZES, ids=IDS)
@pytest.mark.parametrize("mode", MODES)
def test_flow_init_is_the_loop_started_from_ref_plus_it(ftk, mode, size):
    """The loop of model.py:82-95 written out from the public parts, each pinned to its restatement by its own tests."""
    model = models(ftk)[mode]
    (f0, f1, _), _ = frames(size)
    h, w = grid(size)
    init = gaussian_init(size, 3)
    features = model.feature_encoder(torch.cat([f0, f1], dim=0), normalise=True)
    correlation_class = ftk.OnDemandCorrelation if mode == "on_demand" else ftk.CorrelationPyramid
    pyramid = correlation_class(features[:B], features[B:], model.correlation_pyramid_levels, model.correlation_radius)
    inp, net = model.context_encoder(f0, normalise=True)
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    ref = torch.stack([xs, ys], dim=0).float()[None].repeat(B, 1, 1, 1)
    cur = ref + init
    want = []
    for _ in range(ITERATIONS):
        correlation = pyramid.lookup(cur)
        net, mask, delta = model.update_block(net, inp, correlation, cur - ref)
        cur = cur + delta
        want.append(ftk.upsample_flow(cur - ref, mask))
    predictions, flow = model(f0, f1, flow_init=init, return_flow=True)
    assert equal(predictions, want)
    assert P.same(flow.cpu().numpy(), (cur - ref).cpu().numpy())
    assert not equal(predictions, model(f0, f1))  # and the start matters
    assert not P.same(flow.cpu().numpy(), init.cpu().numpy())


@pytest.mark.parametrize("size", SIZES, ids=IDS)
@pytest.mark.parametrize("mode", MODES)
def test_a_cold_tracker_is_pairwise_track_points(ftk, mode, size):
    """The cached-encoder claim: the feature map of a frame encoded alone at batch B is bit for bit its half of the stacked call's."""
    model = models(ftk)[mode]
    (f0, f1, f2), points = frames(size)
    tracker = ftk.RaftVideoTracker(model, warm_start=False)
    assert tracker.track(f0, points) is None and tracker.last_flow is None
    first, second = tracker.track(f1, points), tracker.track(f2, points, return_error=True)
    assert len(first) == 2 and equal(first, model.track_points(f0, f1, points))
    assert len(second) == 3 and second[2] is None and equal(second, model.track_points(f1, f2, points, return_error=True))
    assert P.same(tracker.last_flow.cpu().numpy(), model.track_points(f1, f2, points, return_flow=True)[2].cpu().numpy())
    t = threshold(ftk, mode, size)
    tracker = ftk.RaftVideoTracker(model, warm_start=False, forward_backward=t)
    assert tracker.track(f0) is None
    assert equal(tracker.track(f1, points, return_error=True), model.track_points(f0, f1, points, forward_backward=t, return_error=True))
    assert equal(tracker.track(f2, points), model.track_points(f1, f2, points, forward_backward=t))


@pytest.mark.parametrize("size", SIZES, ids=IDS)
@pytest.mark.parametrize("mode", MODES)
def test_a_warm_tracker_starts_from_the_previous_flow_pushed_forward(ftk, mode, size):
    model = models(ftk)[mode]
    (f0, f1, f2), points = frames(size)
    tracker = ftk.RaftVideoTracker(model)
    assert tracker.track(f0) is None
    cur, status, c01 = model.track_points(f0, f1, points, return_flow=True)
    assert equal(tracker.track(f1, points), (cur, status))  # the first pair starts from zero
    assert P.same(tracker.last_flow.cpu().numpy(), c01.cpu().numpy())
    want = model.track_points(f1, f2, points, flow_init=ftk.warm_start_flow(c01), return_flow=True)
    assert equal(tracker.track(f2, points), want[:2])
    assert P.same(tracker.last_flow.cpu().numpy(), want[2].cpu().numpy())
    cold = model.track_points(f1, f2, points, return_flow=True)
    assert not equal(want[:1], cold[:1]) and not P.same(want[2].cpu().numpy(), cold[2].cpu().numpy())  # the warm start is plugged in


@pytest.mark.parametrize("size", SIZES, ids=IDS)
@pytest.mark.parametrize("mode", MODES)
def test_a_warm_tracker_with_the_check_warms_each_direction(ftk, mode, size):
    model = models(ftk)[mode]
    (f0, f1, f2), points = frames(size)
    t = threshold(ftk, mode, size)
    tracker = ftk.RaftVideoTracker(model, forward_backward=t)
    assert tracker.track(f0) is None
    *result, (forward, backward) = model.track_points(f0, f1, points, forward_backward=t, return_error=True, return_flow=True)
    assert equal(tracker.track(f1, points, return_error=True), result)
    assert equal(tracker.last_flow, (forward, backward))
    inits = (ftk.warm_start_flow(forward), ftk.warm_start_flow(backward))
    *want, flows = model.track_points(f1, f2, points, forward_backward=t, return_error=True, flow_init=inits, return_flow=True)
    got = tracker.track(f2, points, return_error=True)
    assert equal(got, want) and equal(tracker.last_flow, flows)
    cold = model.track_points(f1, f2, points, forward_backward=t, return_error=True)
    assert not equal(got[:1], cold[:1])


def test_reset_points_none_and_a_frame_of_another_shape(ftk):
    model = models(ftk)["all_pairs"]
    (f0, f1, f2), points = frames(SIZES[0])
    tracker = ftk.RaftVideoTracker(model, iterations=ITERATIONS)
    assert tracker.track(f0) is None
    assert tracker.track(f1) is None  # points=None advances the state
    c01 = model.track_points(f0, f1, points, return_flow=True)[2]
    assert P.same(tracker.last_flow.cpu().numpy(), c01.cpu().numpy())
    want = model.track_points(f1, f2, points, flow_init=ftk.warm_start_flow(c01))
    assert equal(tracker.track(f2, points), want)
    other = frames(SIZES[1])[0][0]
    before = tracker.last_flow
    for bad in (other, f0[:1], f0.double()):
        with pytest.raises(ValueError, match="image must be|call reset\\(\\)") as e:
            tracker.track(bad, points)
        if bad.dtype == torch.float32:
            assert str(list(bad.shape)) in str(e.value) and str(list(f0.shape)) in str(e.value) and "reset()" in str(e.value)
    assert tracker.last_flow is before  # a refused frame changes nothing
    with pytest.raises(ValueError, match="points must be"):
        tracker.track(f0, points[:, :, :1])
    assert tracker.last_flow is before
    tracker.reset()
    assert tracker.last_flow is None and tracker.track(other) is None  # another shape after a reset
    tracker.reset()
    assert tracker.track(f1, points) is None  # a first call again, points or not
    assert equal(tracker.track(f2, points), model.track_points(f1, f2, points))  # and the first pair starts from zero
    # a stored frame is the tracker's own: overwriting the caller's tensor afterwards changes nothing
    tracker.reset()
    mine = f1.clone()
    tracker.track(mine)
    mine.fill_(0.0)
    assert equal(tracker.track(f2, points), model.track_points(f1, f2, points))


class CountingLib:
    """Stands in front of the loaded library and counts the device entries it is asked for."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        entry = getattr(self._lib, name)
        if name.endswith("_device"):
            self.calls.append(name)
        return entry


def test_library_entries_per_frame(ftk, monkeypatch):
    """The docstring's count, in entries of the library (an entry is one launch, except the correlation build beyond four levels and
    warm_start_flow's two launches in one entry): a frame of the tracker enters it as often as pairwise track_points does, the feature
    encoder's 17 among them at batch B, plus once for the warm start from the second pair on; points=None saves the points entry and
    the mask head's two."""
    from feature_tracker_amd import _native as N
    model = models(ftk)["all_pairs"]
    (f0, f1, f2), points = frames(SIZES[0])
    counting = CountingLib(N.lib())
    monkeypatch.setattr(N, "lib", lambda: counting)

    def entries(call):
        counting.calls.clear()
        call()
        return list(counting.calls)

    n = ITERATIONS
    pairwise = entries(lambda: model.track_points(f0, f1, points))
    assert len(pairwise) == 36 + 14 * n - 2 * (n - 1) + 1
    tracker = ftk.RaftVideoTracker(model)
    assert len(entries(lambda: tracker.track(f0))) == 17
    assert sorted(entries(lambda: tracker.track(f1, points))) == sorted(pairwise)
    warm = entries(lambda: tracker.track(f2, points))
    assert sorted(warm) == sorted(pairwise + ["ftk_flow_warm_device"])
    assert len(entries(lambda: tracker.track(f1))) == len(warm) - 3
    checked = ftk.RaftVideoTracker(model, forward_backward=1.0)
    checked.track(f0)
    checked.track(f1)
    assert sorted(entries(lambda: checked.track(f2, points))) == sorted(warm)  # one warm start over both directions
