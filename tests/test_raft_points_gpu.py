"""Raft.track_points on the device: bit for bit what Raft.__call__'s last prediction gives when it is copied to the host
and put through the restatement's sampling and status rules (tests/flow_points_ref.c), in both correlation modes, with and without the
forward-backward check (whose backward half is Raft.__call__ on the swapped pair: the loop at batch 2B changes no bit); UpdateBlock's
``want_mask=False``; and graph capture.  The model is the reference's configuration (model.py:105-117) at seeded random weights."""
import functools

import numpy as np
import pytest

from tests import flow_points_ref as P
from tests import raft_conv_ref
from tests.test_flow_points_cpu import point_set
from tests.test_raft_encoder_cpu import RAFT_CASES, make_image, make_raft_state

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WIDTHS = RAFT_CASES[2][:11]  # model.py:105-117's
SIZES = [(60, 60), (44, 68)]  # 60 x 60 gives a 64 x 64 grid: the image is smaller than it; 44 x 68 gives 48 x 72
B, ITERATIONS, COUNT = 2, 2, 150


def on_device(a):
    a = a.numpy() if hasattr(a, "numpy") else a
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


@functools.lru_cache(maxsize=None)
def models(ftk):
    state = {k: on_device(v) for k, v in make_raft_state(WIDTHS, 1).items()}
    return {mode: ftk.Raft.from_state_dict(state, WIDTHS[3], WIDTHS[4], max_iterations=ITERATIONS, correlation=mode) for mode in ("all_pairs", "on_demand")}


@functools.lru_cache(maxsize=None)
def dense_case(ftk, mode, size):
    """(ref_image, cur_image, points on the device; points, the forward and the backward last prediction on the host), computed once."""
    H, W = size
    ref_image, cur_image = on_device(make_image(B, 1, H, W, 21)), on_device(make_image(B, 1, H, W, 22))
    h, w = ((((e + 1) // 2 + 1) // 2 + 1) // 2 for e in size)
    points = point_set(B, h, w, COUNT, size, 13)
    model = models(ftk)[mode]
    forward = model(ref_image, cur_image)[-1].cpu().numpy()
    backward = model(cur_image, ref_image)[-1].cpu().numpy()
    assert forward.shape == (B, 2, 8 * h, 8 * w)
    return ref_image, cur_image, on_device(points), points, forward, backward


@pytest.mark.parametrize("size", SIZES, ids=["60x60", "44x68"])
@pytest.mark.parametrize("mode", ["all_pairs", "on_demand"])
def test_track_points_is_the_last_prediction_sampled(ftk, mode, size):
    ref_image, cur_image, points, host_points, forward, _ = dense_case(ftk, mode, size)
    want = P.track_dense(forward, host_points, size)
    got = models(ftk)[mode].track_points(ref_image, cur_image, points)
    assert len(got) == 2 and got[0].shape == (B, COUNT, 2) and got[1].dtype == torch.uint8
    assert P.same(got[0].cpu().numpy(), want[0]) and P.same(got[1].cpu().numpy(), want[1])
    assert {P.TRACKED, P.OUTSIDE} <= set(np.unique(want[1]).tolist())
    cur, status, e2 = models(ftk)[mode].track_points(ref_image, cur_image, points, iterations=ITERATIONS, return_error=True)
    assert e2 is None and P.same(cur.cpu().numpy(), want[0]) and P.same(status.cpu().numpy(), want[1])


@pytest.mark.parametrize("size", SIZES, ids=["60x60", "44x68"])
@pytest.mark.parametrize("mode", ["all_pairs", "on_demand"])
def test_forward_backward_is_the_swapped_pair_sampled(ftk, mode, size):
    ref_image, cur_image, points, host_points, forward, backward = dense_case(ftk, mode, size)
    # a threshold that separates the points: the median forward-backward distance of the restated result
    _, _, every = P.track_dense(forward, host_points, size, backward, float("inf"))
    t = float(np.sqrt(np.median(every[every > 0])))
    want = P.track_dense(forward, host_points, size, backward, t)
    assert {P.TRACKED, P.LARGE_RESIDUAL, P.OUTSIDE} <= set(np.unique(want[1]).tolist())
    model = models(ftk)[mode]
    got = [g.cpu().numpy() for g in model.track_points(ref_image, cur_image, points, forward_backward=t, return_error=True)]
    assert all(P.same(g, w) for g, w in zip(got, want)), [P.same(g, w) for g, w in zip(got, want)]
    assert len(model.track_points(ref_image, cur_image, points, forward_backward=t)) == 2
    plain = [g.cpu().numpy() for g in model.track_points(ref_image, cur_image, points)]
    kept = got[1] != P.LARGE_RESIDUAL
    assert P.same(got[0][kept], plain[0][kept]) and P.same(got[1][kept], plain[1][kept])


def test_update_block_without_the_mask_head(ftk):
    c = RAFT_CASES[1]
    state = make_raft_state(c, 3)
    block = ftk.UpdateBlock.from_state_dict({k: on_device(v) for k, v in state.items()})
    rng = np.random.default_rng(5)
    widths = (c[0], c[2], c[3] * (2 * c[4] + 1) ** 2, 2)
    net, inp, correlation, flow = (rng.standard_normal((2, ch, 5, 35)).astype(np.float32) for ch in widths)
    args = [on_device(a) for a in (net, inp, correlation, flow)]
    default = block(*args)
    new_net, mask, delta = block(*args, want_mask=False)
    assert mask is None
    assert P.same(new_net.cpu().numpy(), default[0].cpu().numpy()) and P.same(delta.cpu().numpy(), default[2].cpu().numpy())
    want = raft_conv_ref.update_block(net, inp, correlation, flow, raft_conv_ref.weights_of(state, "update_block."))[:3]
    assert all(P.same(g.cpu().numpy(), w) for g, w in zip(default, want))  # the default call is what it was
    assert all(P.same(g.cpu().numpy(), w) for g, w in zip(block(*args, want_mask=True), want))


def test_graph_capture_and_two_replays(ftk):
    """track_points with the check, recorded in torch.cuda.graph on a single stream and replayed twice with images and points overwritten
    in place: each replay equals the eager result on the same inputs bit for bit."""
    c = RAFT_CASES[0]
    _, H, W, iterations = c[11:]
    model = ftk.Raft.from_state_dict({k: on_device(v) for k, v in make_raft_state(c, 1).items()}, c[3], c[4], max_iterations=iterations)
    h, w = ((((e + 1) // 2 + 1) // 2 + 1) // 2 for e in (H, W))
    sets = [(on_device(make_image(1, 1, H, W, 30 + n)), on_device(make_image(1, 1, H, W, 40 + n)), on_device(point_set(1, h, w, 70, (H, W), n))) for n in range(3)]
    eager = [[g.cpu().numpy() for g in model.track_points(*s, forward_backward=1.0, return_error=True)] for s in sets]
    held = [t.clone() for t in sets[0]]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        model.track_points(*held, forward_backward=1.0, return_error=True)  # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = model.track_points(*held, forward_backward=1.0, return_error=True)
    for n in (1, 2):
        for dst, src in zip(held, sets[n]):
            dst.copy_(src)
        out[0].fill_(float("nan"))
        out[1].fill_(255)
        out[2].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert all(P.same(o.cpu().numpy(), e) for o, e in zip(out, eager[n])), f"replay {n}"
