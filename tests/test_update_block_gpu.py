"""conv2d_kernel, MotionEncoder and UpdateBlock on the device against the scalar restatement (tests/raft_conv_ref.c): bit-identical on
every shape, channel count and kernel size (any NaN equals any NaN); the torch composition of update_block.py:61-67
on the same device agrees within the CPU test's bound.  The shapes are the smallest that reach each edge of a tile of 32 output
channels x 32 pixels x wn rows (wn = 4, 2, 1 for 1, 2, >= 3 tiles of output channels) and of a chunk of 32 / 8 / 2 input channels."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import raft_conv_ref as R
from tests.test_update_block_cpu import BOUND, CASES, make_inputs, make_state, torch_forward

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from feature_tracker_amd import _native as N  # noqa: E402

# (C_in, C_out, kernel_size, relu, scale, B, H, W)
CONV_SHAPES = [
    (16, 2, 3, False, 1.0, 1, 4, 5), (5, 33, 3, True, 1.0, 1, 4, 5), (40, 576, 1, False, 0.25, 1, 3, 5),  # a partial tile of output channels
    (3, 16, 3, True, 1.0, 1, 3, 4), (131, 8, 3, True, 1.0, 1, 3, 4), (33, 8, 1, True, 1.0, 1, 3, 4),       # odd K, a partial last chunk
    (2, 8, 7, True, 1.0, 1, 5, 6), (3, 8, 7, False, 1.0, 1, 5, 6),                                          # the flow's 7 x 7; an odd K of it
    (2, 8, 7, True, 1.0, 1, 1, 1), (2, 8, 7, True, 1.0, 1, 1, 7), (2, 8, 7, True, 1.0, 1, 7, 1), (2, 8, 7, True, 1.0, 1, 3, 3),  # smaller than the kernel
    (9, 8, 3, True, 1.0, 1, 1, 1), (9, 40, 3, True, 1.0, 1, 2, 1), (9, 8, 1, False, 1.0, 1, 1, 1),
    (6, 16, 3, True, 1.0, 1, 9, 35), (6, 16, 1, True, 1.0, 1, 5, 35), (2, 16, 7, True, 1.0, 1, 9, 35),      # wn 4: W and H beyond a tile by a non-multiple
    (6, 48, 3, True, 1.0, 1, 5, 67), (6, 48, 1, False, 0.25, 1, 9, 67), (2, 48, 7, True, 1.0, 1, 5, 67),    # wn 2
    (6, 100, 3, True, 1.0, 1, 5, 131), (6, 100, 1, True, 1.0, 1, 9, 131), (2, 100, 7, False, 1.0, 1, 5, 131),  # wn 1
    (10, 40, 3, True, 1.0, 2, 5, 9), (2, 40, 7, True, 1.0, 2, 5, 9), (40, 40, 1, True, 1.0, 2, 5, 9),       # B = 2
]
# the CPU test's three cases and one whose width is beyond a tile by a non-multiple, with 2 tiles of most channel counts
BLOCK_CASES = CASES + [(40, 6, 20, 40, 33, 24, 12, 34, 40, 1, 5, 37)]


def where_differs(got, want):
    return np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5].tolist()


def on_device(t):
    return torch.from_numpy(np.ascontiguousarray(t)).to("cuda")


def make_conv(Cin, Cout, ks, B, H, W, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, ks, ks)) / np.sqrt(Cin * ks * ks)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    return x, w, b


def run_conv(parts, weight, bias, relu, scale=1.0):
    """conv2d_device on numpy operands: packs as raft.py does, launches on torch's current stream, returns the result on the host."""
    from feature_tracker_amd import device as D
    from feature_tracker_amd import raft
    parts = [parts] if isinstance(parts, np.ndarray) else list(parts)
    parts = [on_device(p) for p in parts]
    B, _, H, W = parts[0].shape
    out = torch.full((B, weight.shape[0], H, W), float("nan"), device="cuda")
    ctx = raft._context(torch.cuda.current_device())
    D.conv2d_device(ctx, parts, raft._pack_conv(on_device(weight)), on_device(bias), weight.shape[2], relu, scale, out)
    return out.cpu().numpy()


@pytest.mark.parametrize("Cin,Cout,ks,relu,scale,B,H,W", CONV_SHAPES, ids=[str(s) for s in CONV_SHAPES])
def test_conv2d_bit_identical_to_the_restatement(ftk, Cin, Cout, ks, relu, scale, B, H, W):
    x, w, b = make_conv(Cin, Cout, ks, B, H, W, 11)
    got = run_conv(x, w, b, relu, scale)
    want = R.conv2d(x, w, b, relu, scale)
    assert got.shape == (B, Cout, H, W)
    assert R.same(got, want), f"differs at {where_differs(got, want)}"


@pytest.mark.parametrize("ks", [1, 3, 7])
def test_parts_that_cross_a_chunk_boundary(ftk, ks):
    """Parts of 3, 30 and 2 channels (chunks of 32, 8 and 2: the second part crosses a boundary) against the concatenated call."""
    x, w, b = make_conv(35, 40, ks, 2, 5, 37, 12)
    whole = run_conv(x, w, b, True)
    parts = run_conv((x[:, :3], x[:, 3:33], x[:, 33:]), w, b, True)
    assert R.same(parts, whole), where_differs(parts, whole)
    assert R.same(whole, R.conv2d(x, w, b, True))


# ---- MotionEncoder and UpdateBlock -----------------------------------------------------------------------------------------------


def device_block(ftk, state):
    return ftk.UpdateBlock.from_state_dict({k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)).to("cuda") for k, v in state.items()}, prefix="")


@functools.lru_cache(maxsize=None)
def block_case(k):
    """(state, inputs, the restatement's (new_net, mask, delta_flow, features)) of BLOCK_CASES[k]: computed once; nobody writes to them."""
    widths, (B, H, W) = BLOCK_CASES[k][:9], BLOCK_CASES[k][9:]
    state = make_state(widths, 11)
    inputs = make_inputs(widths, B, H, W, 11)
    return state, inputs, R.update_block(*(t.numpy() for t in inputs), R.weights_of(state))


@pytest.mark.parametrize("k", range(len(BLOCK_CASES)), ids=[str(c) for c in BLOCK_CASES])
def test_update_block_bit_identical_and_within_the_bound_of_torch(ftk, k):
    state, inputs, want = block_case(k)
    block = device_block(ftk, state)
    net, inp, corr, flow = (t.to("cuda") for t in inputs)
    features = block.motion_encoder.features(corr, flow)
    motion = block.motion_encoder(corr, flow)
    got = block(net, inp, corr, flow)
    assert R.same(features.cpu().numpy(), want[3]), f"features differ at {where_differs(features.cpu().numpy(), want[3])}"
    assert R.same(motion.cpu().numpy(), np.concatenate([want[3], inputs[3].numpy()], axis=1))
    for name, g, w in zip(("new_net", "mask", "delta_flow"), got, want):
        assert g.shape == w.shape and g.is_contiguous()
        assert R.same(g.cpu().numpy(), w), f"{name} differs at {where_differs(g.cpu().numpy(), w)}"
    # stock torch ops on the same device: their convolutions sum in their own order, so not bit-identical
    dev_state = {key: v.to("cuda") for key, v in state.items()}
    ref64 = torch_forward(dev_state, net, inp, corr, flow, torch.float64)[:3]
    ref32 = torch_forward(dev_state, net, inp, corr, flow)[:3]
    ours = max(float((g.double() - r).abs().max()) for g, r in zip(got, ref64))
    theirs = max(float((t.double() - r).abs().max()) for t, r in zip(ref32, ref64))
    apart = max(float((g - t).abs().max()) for g, t in zip(got, ref32))
    print(f"UpdateBlock vs float64 {ours:.3g}, torch float32 vs float64 {theirs:.3g}, each other {apart:.3g} (bound {BOUND:.3g})")
    assert ours <= BOUND
    assert apart <= BOUND


def test_hostile_values(ftk):
    """A NaN and an inf at one input pixel each, -0 biases, and pre-activations of +-200: NaNs at exactly the restatement's positions."""
    widths, (B, H, W) = CASES[0][:9], (1, 6, 40)
    state = {k: v.clone() for k, v in make_state(widths, 13).items()}
    for k in state:
        if k.endswith(".bias"):
            state[k][::3] = -0.0
    state["motion_encoder.correlation_conv.0.bias"][1], state["motion_encoder.correlation_conv.2.bias"][2] = 200.0, -200.0
    state["motion_encoder.flow_conv.0.bias"][4], state["motion_encoder.out_conv.0.bias"][5] = -200.0, 200.0
    state["flow_head.conv1.bias"][1], state["mask.0.bias"][2], state["mask.2.bias"][7], state["flow_head.conv2.bias"][1] = 200.0, -200.0, 200.0, -200.0
    net, inp, corr, flow = (t.numpy().copy() for t in make_inputs(widths, B, H, W, 13))
    corr[0, 2, 1, 3] = np.nan
    flow[0, 1, 4, 5] = np.inf
    got = [t.cpu().numpy() for t in device_block(ftk, state)(*(on_device(t) for t in (net, inp, corr, flow)))]
    want = R.update_block(net, inp, corr, flow, R.weights_of(state))[:3]
    for name, g, w in zip(("new_net", "mask", "delta_flow"), got, want):
        assert np.isnan(w).any() and not np.isnan(w).all(), name
        assert np.array_equal(np.isnan(g), np.isnan(w)), name
        assert R.same(g, w), (name, where_differs(g, w))
    # one layer, where ReLU meets the special values directly: -0 and NaN pass, negatives become +0, then the scale
    x = np.float32([-0.0, np.nan, -3.0, np.inf, -np.inf, 5.0, 0.0]).reshape(1, 1, 1, 7)
    for w in (np.ones((1, 1, 1, 1), np.float32), -np.ones((1, 1, 1, 1), np.float32)):
        for relu, scale in ((True, 1.0), (True, -0.25), (False, 0.25)):
            bias = np.float32([-0.0])
            g, r = run_conv(x, w, bias, relu, scale), R.conv2d(x, w, bias, relu, scale)
            assert R.same(g, r), (relu, scale, g, r)


@pytest.mark.parametrize("ks", [1, 3, 7])
def test_subnormal_weights_times_subnormal_inputs(ftk, ks):
    """The matrix cores do not flush their A / B operands: with zero biases and every input subnormal, each result is a chain of
    subnormal products (ordinary weights) and of products that underflow to 0 (the subnormal weights of channel 0)."""
    x, w, b = make_conv(4, 16, ks, 1, 3, 5, 14)
    w[:, 0] *= np.float32(2e-39)
    x *= np.float32(3e-39)
    b[:] = 0
    tiny = np.finfo(np.float32).tiny
    assert (np.abs(x) < tiny).all() and (np.abs(w[:, 0]) < tiny).all()
    got, want = run_conv(x, w, b, False), R.conv2d(x, w, b, False)
    assert ((np.abs(want) < tiny) & (want != 0)).mean() > 0.9  # flushing any operand would change the result
    assert R.same(got, want), where_differs(got, want)


def test_inputs_unchanged_and_non_contiguous_inputs(ftk):
    state, inputs, want = block_case(0)
    block = device_block(ftk, state)
    dense = [t.to("cuda") for t in inputs]
    strided = [t.transpose(2, 3).contiguous().transpose(2, 3) for t in dense]
    assert not any(t.is_contiguous() for t in strided)
    got = block(*strided)
    for g, w in zip(got, want):
        assert g.is_contiguous() and g.data_ptr() not in [t.data_ptr() for t in dense + strided]
        assert R.same(g.cpu().numpy(), w)
    features = block.motion_encoder.features(strided[2], strided[3])
    assert features.is_contiguous() and R.same(features.cpu().numpy(), want[3])
    for d, s, t in zip(dense, strided, inputs):
        assert torch.equal(d.cpu(), t) and torch.equal(s.cpu(), t)


def test_graph_capture_and_replay(ftk):
    """One UpdateBlock call recorded in torch.cuda.graph on a single stream, replayed with the inputs overwritten in place: the replay
    equals the eager result on the same inputs bit for bit."""
    widths, (B, H, W) = BLOCK_CASES[3][:9], BLOCK_CASES[3][9:]
    block = device_block(ftk, make_state(widths, 16))
    sets = [tuple(t.to("cuda") for t in make_inputs(widths, B, H, W, 20 + n)) for n in range(2)]
    eager = [[t.cpu().numpy() for t in block(*s)] for s in sets]
    held = [t.clone() for t in sets[0]]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        block(*held)  # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = block(*held)
    for h, s in zip(held, sets[1]):
        h.copy_(s)
    for o in out:
        o.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for name, o, e in zip(("new_net", "mask", "delta_flow"), out, eager[1]):
        assert R.same(o.cpu().numpy(), e), name


def test_inference_only_and_native_refusals(ftk):
    from feature_tracker_amd import raft
    state, inputs, _ = block_case(0)
    block = device_block(ftk, state)
    net, inp, corr, flow = (t.to("cuda") for t in inputs)
    with pytest.raises(RuntimeError, match="inference only"):
        block(net, inp, corr, flow.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="net must be"):
        block(net[:, :15], inp, corr, flow)
    # the C entry itself: sizes above the stated limits are FTK_E_UNSUPPORTED, recorded before any launch
    ctx = raft._context(torch.cuda.current_device())
    B, _, H, W = net.shape
    out = torch.full((B, 8, H, W), 7.0, device="cuda")
    weights, bias, ks, M = block._layers["mask.0"]
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    part = lambda channels: (N.GruPart * 1)(N.GruPart(ptr(net), channels))  # noqa: E731

    def conv(parts, n_parts, out_channels, kernel_size, scale=1.0, sizes=(B, H, W)):
        return N.lib().ftk_conv2d_device(ctx.handle, None, parts, n_parts, ptr(weights), ptr(bias), out_channels, kernel_size, 1, scale, *sizes, ptr(out))

    for args, code, match in (((part(16), 1, N.FTK_CONV2D_MAX_OUT_CHANNELS + 1, 3), -4, "FTK_CONV2D_MAX_OUT_CHANNELS"),
                              ((part(N.FTK_CONV2D_MAX_IN_CHANNELS + 1), 1, 8, 3), -4, "FTK_CONV2D_MAX_IN_CHANNELS"),
                              ((part(16), 1, 8, 5), -4, "kernel_size 5"), ((part(16), 4, 8, 3), -1, "parts"), ((part(0), 1, 8, 3), -1, "part 0"),
                              ((part(16), 1, 8, 3, float("inf")), -1, "out_scale"), ((part(16), 1, 8, 3, 1.0, (B, 0, W)), -1, "positive")):
        rc = conv(*args)
        assert rc == code, (args[1:], rc)
        with pytest.raises(N.FtkError, match=match):
            N.check(rc, ctx.handle)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
