"""SepConvGru on the device against the scalar restatement (tests/sep_conv_gru_ref.c): bit-identical on every shape, channel count and
kernel size (any NaN equals any NaN); the torch composition of gru.py:59-76 on the same device agrees within the CPU
test's bound."""
import ctypes as C

import numpy as np
import pytest

from tests import sep_conv_gru_ref as R
from tests.test_sep_conv_gru_cpu import BOUND, make_inputs, make_state, torch_forward

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from feature_tracker_amd import _native as N  # noqa: E402

# (x_channels, h_channels, kernel_size, B, H, W).  A workgroup's strip is 32 wn pixels of a row (horizontal) or wn rows of 32 pixels
# (vertical), wn = 4, 2, 1 for 1, 2, >= 3 tiles of 32 output channels; a chunk is 16 input channels.
SHAPES = [
    (3, 16, 5, 2, 6, 7), (160, 64, 5, 2, 6, 7), (131, 256, 5, 2, 6, 7),  # the reference's three configurations
    (3, 1, 5, 1, 4, 5), (2, 33, 5, 1, 4, 5), (3, 40, 3, 1, 4, 5),         # a partial tile of output channels: 1 (2), 33 (66), 40 (80)
    (1, 16, 5, 1, 3, 4), (131, 8, 3, 1, 3, 4),                            # odd K: 17 * 5, 139 * 3
    (3, 16, 5, 1, 1, 1), (3, 16, 3, 1, 1, 7), (3, 16, 5, 1, 7, 1), (5, 48, 5, 1, 3, 3), (4, 16, 3, 1, 2, 131),  # narrower / shorter than the kernel
    (3, 16, 5, 1, 9, 133), (3, 48, 3, 1, 7, 67), (6, 100, 5, 2, 3, 35),   # W and H beyond one strip by a non-multiple, for wn = 4, 2, 1
]


def where_differs(got, want):
    return np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5].tolist()


def on_device(t):
    return torch.from_numpy(np.ascontiguousarray(t)).to("cuda")


def device_gru(ftk, state):
    return ftk.SepConvGru.from_state_dict({k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)).to("cuda") for k, v in state.items()})


def run(ftk, state, x, h):
    gru = device_gru(ftk, state)
    xs = on_device(x) if isinstance(x, np.ndarray) else [on_device(p) for p in x]
    return gru(xs, on_device(h)).cpu().numpy()


@pytest.mark.parametrize("Cx,Ch,ks,B,H,W", SHAPES, ids=[str(s) for s in SHAPES])
def test_bit_identical_to_the_restatement(ftk, Cx, Ch, ks, B, H, W):
    state = make_state(Cx, Ch, ks, 11)
    x, h = (t.numpy() for t in make_inputs(Cx, Ch, B, H, W, 11))
    got = run(ftk, state, x, h)
    want = R.forward(x, h, R.weights_of(state))
    assert got.shape == (B, Ch, H, W)
    assert R.same(got, want), f"differs at {where_differs(got, want)}"


def test_three_parts_equal_the_concatenation(ftk):
    """Parts of 3, 30 and 2 channels (the second crosses a chunk boundary) against the concatenated call and the restatement."""
    state = make_state(35, 40, 5, 12)
    x, h = (t.numpy() for t in make_inputs(35, 40, 2, 5, 37, 12))
    whole = run(ftk, state, x, h)
    parts = run(ftk, state, (x[:, :3], x[:, 3:33], x[:, 33:]), h)
    assert R.same(parts, whole), where_differs(parts, whole)
    assert R.same(whole, R.forward(x, h, R.weights_of(state)))


def test_hostile_values(ftk):
    """A NaN and an inf at one input pixel each, -0 biases, and pre-activations of +-200: NaNs at exactly the restatement's positions."""
    Cx, Ch, ks, B, H, W = 5, 40, 5, 1, 6, 40
    state = {k: v.clone() for k, v in make_state(Cx, Ch, ks, 13).items()}
    for g in R.GATES:
        state[f"conv_{g}.bias"][::3] = -0.0
    state["conv_z_horizontal.bias"][1], state["conv_z_horizontal.bias"][2] = 200.0, -200.0
    state["conv_r_vertical.bias"][4], state["conv_q_vertical.bias"][5], state["conv_q_horizontal.bias"][7] = -200.0, 200.0, -200.0
    x, h = (t.numpy().copy() for t in make_inputs(Cx, Ch, B, H, W, 13))
    x[0, 2, 1, 3] = np.nan
    h[0, 17, 4, 33] = np.inf
    got = run(ftk, state, x, h)
    want = R.forward(x, h, R.weights_of(state))
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert R.same(got, want), where_differs(got, want)


def test_subnormal_weights_times_subnormal_inputs(ftk):
    """The matrix cores do not flush their A / B operands.  With h = 0, zero biases and every x subnormal, each pre-activation is a
    chain of subnormal products (ordinary weights), of products that underflow to 0 (the subnormal weights of channel 0) and, for z of
    the horizontal pass, of normal ones (weights of 2^20); q and the new h stay subnormal through both passes."""
    Cx, Ch, ks, B, H, W = 4, 16, 3, 1, 3, 5
    state = {k: v.clone() for k, v in make_state(Cx, Ch, ks, 14).items()}
    for g in R.GATES:
        state[f"conv_{g}.bias"].zero_()
        state[f"conv_{g}.weight"][:, 0] *= 2e-39  # subnormal weights
    state["conv_z_horizontal.weight"][:, 1:Cx] *= 2.0 ** 20
    x, h = (t.numpy().copy() for t in make_inputs(Cx, Ch, B, H, W, 14))
    x *= np.float32(3e-39)
    h[:] = 0
    tiny = np.finfo(np.float32).tiny
    assert (np.abs(x) < tiny).all() and (np.abs(state["conv_q_vertical.weight"][:, 0].numpy()) < tiny).all()
    got = run(ftk, state, x, h)
    want = R.forward(x, h, R.weights_of(state))
    assert ((np.abs(want) < tiny) & (want != 0)).mean() > 0.9  # flushing any operand would change the result
    assert R.same(got, want), where_differs(got, want)


def test_inputs_unchanged_and_non_contiguous_inputs(ftk):
    state = make_state(6, 16, 5, 15)
    x, h = make_inputs(6, 16, 2, 5, 9, 15)
    want = R.forward(x.numpy(), h.numpy(), R.weights_of(state))
    gru = device_gru(ftk, state)
    xd, hd = x.to("cuda"), h.to("cuda")
    x_t = xd.transpose(2, 3).contiguous().transpose(2, 3)
    h_t = hd.transpose(2, 3).contiguous().transpose(2, 3)
    assert not x_t.is_contiguous() and not h_t.is_contiguous()
    parts = (x_t[:, :1], x_t[:, 1:4], xd[:, 4:])  # channel slices of a strided and of a dense tensor
    out = gru(parts, h_t)
    assert out.data_ptr() not in (h_t.data_ptr(), hd.data_ptr()) and out.is_contiguous()
    assert R.same(out.cpu().numpy(), want)
    assert torch.equal(xd.cpu(), x) and torch.equal(hd.cpu(), h) and torch.equal(x_t.cpu(), x) and torch.equal(h_t.cpu(), h)


def test_graph_capture_and_two_replays(ftk):
    """One call recorded in torch.cuda.graph on a single stream, replayed twice with the inputs overwritten in place in between: each
    replay equals the eager result on the same inputs bit for bit."""
    Cx, Ch, ks, B, H, W = 6, 40, 5, 1, 5, 37
    gru = device_gru(ftk, make_state(Cx, Ch, ks, 16))
    sets = [tuple(t.to("cuda") for t in make_inputs(Cx, Ch, B, H, W, 20 + n)) for n in range(3)]
    eager = [gru((x[:, :2], x[:, 2:]), h).cpu().numpy() for x, h in sets]
    x, h = sets[0][0].clone(), sets[0][1].clone()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        gru((x[:, :2], x[:, 2:]), h)  # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = gru((x[:, :2], x[:, 2:]), h)
    for n in (1, 2):
        x.copy_(sets[n][0])
        h.copy_(sets[n][1])
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert R.same(out.cpu().numpy(), eager[n]), f"replay {n}"


def test_against_the_torch_composition_on_the_device(ftk):
    """Stock torch ops (gru.py:59-76) in float32 on the same device: its convolutions sum in their own order, so not bit-identical;
    both sides are within the CPU test's bound of the float64 composition, hence within twice it of each other."""
    Cx, Ch, ks, B, H, W = 131, 64, 5, 2, 12, 45
    state = make_state(Cx, Ch, ks, 17)
    x, h = make_inputs(Cx, Ch, B, H, W, 17)
    dev_state = {k: v.to("cuda") for k, v in state.items()}
    got = device_gru(ftk, state)(x.to("cuda"), h.to("cuda"))
    ref64 = torch_forward(dev_state, x.to("cuda"), h.to("cuda"), torch.float64)
    ref32 = torch_forward(dev_state, x.to("cuda"), h.to("cuda"))
    ours, theirs = float((got.double() - ref64).abs().max()), float((ref32.double() - ref64).abs().max())
    print(f"SepConvGru vs float64 {ours:.3g}, torch float32 vs float64 {theirs:.3g}, each other {float((got - ref32).abs().max()):.3g} (bound {BOUND:.3g})")
    assert ours <= BOUND
    assert float((got - ref32).abs().max()) <= 2 * BOUND


def test_inference_only_and_native_refusals(ftk):
    from feature_tracker_amd import raft
    state = make_state(3, 16, 5, 18)
    gru = device_gru(ftk, state)
    x, h = (t.to("cuda") for t in make_inputs(3, 16, 1, 4, 5, 18))
    with pytest.raises(RuntimeError, match="inference only"):
        gru(x, h.clone().requires_grad_(True))
    with torch.no_grad():
        assert R.same(gru(x, h.clone().requires_grad_(True)).cpu().numpy(), gru(x, h).cpu().numpy())
    # the C entries themselves: sizes above the stated limits are FTK_E_UNSUPPORTED, recorded before any launch
    ctx = raft._context(torch.cuda.current_device())
    z, rh, out = (torch.full((1, 16, 4, 5), 7.0, device="cuda") for _ in range(3))
    p = gru._packed
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    part = lambda channels: (N.GruPart * 1)(N.GruPart(ptr(x), channels))  # noqa: E731
    lib = N.lib()

    def gates(parts, n_parts, h_channels, ks, sizes=(1, 4, 5)):
        return lib.ftk_sep_conv_gru_gates_device(ctx.handle, None, parts, n_parts, ptr(h), ptr(p["zr_horizontal"]), ptr(p["zr_bias_horizontal"]), h_channels, ks,
                                                 0, *sizes, ptr(z), ptr(rh))

    def blend(parts, n_parts, h_channels, ks, sizes=(1, 4, 5)):
        return lib.ftk_sep_conv_gru_blend_device(ctx.handle, None, parts, n_parts, ptr(rh), ptr(z), ptr(h), ptr(p["q_horizontal"]), ptr(p["q_bias_horizontal"]),
                                                 h_channels, ks, 0, *sizes, ptr(out))

    for entry in (gates, blend):
        for args, code, match in (((part(3), 1, N.FTK_SEP_CONV_GRU_MAX_H_CHANNELS + 1, 5), -4, "FTK_SEP_CONV_GRU_MAX_H_CHANNELS"),
                                  ((part(N.FTK_SEP_CONV_GRU_MAX_IN_CHANNELS - 15), 1, 16, 5), -4, "FTK_SEP_CONV_GRU_MAX_IN_CHANNELS"),
                                  ((part(3), 1, 16, 7), -4, "kernel_size 7"), ((part(3), 4, 16, 5), -1, "parts"), ((part(0), 1, 16, 5), -1, "part 0"),
                                  ((part(3), 1, 16, 5, (1, 0, 5)), -1, "positive")):
            rc = entry(*args)
            assert rc == code, (entry.__name__, args[1:], rc)
            with pytest.raises(N.FtkError, match=match):
                N.check(rc, ctx.handle)
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((rh == 7.0).all()) and bool((out == 7.0).all())  # nothing was launched


def test_tensors_on_two_devices(ftk):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second HIP device")
    gru = ftk.SepConvGru.from_state_dict({k: v.to("cuda:0") for k, v in make_state(3, 16, 5, 19).items()})
    x, h = make_inputs(3, 16, 1, 4, 5, 19)
    with pytest.raises(ValueError, match="device"):
        gru(x.to("cuda:0"), h.to("cuda:1"))
    with pytest.raises(ValueError, match="weights are on"):
        gru(x.to("cuda:1"), h.to("cuda:1"))
