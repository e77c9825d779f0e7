"""RAFT's UpdateBlock without a device: the scalar restatement (tests/raft_conv_ref.c around tests/sep_conv_gru_ref.c)
pinned against an independent float64 composition of update_block.py:61-67 (torch.nn.functional.conv2d / relu / cat in float64, written
out below), six mutants of the restatement that the same bound must reject, a golden fixture recorded from the reference's own module,
known answers that need no float64 side, the packed layout, the loud failures of the Python entries before any device is touched, and
the launch plan through its command-line tool.

Measured (printed by the tests, -s shows them): restatement against float64 over CASES x MEASURED_SEEDS, the largest absolute
difference of the three outputs: 4.18e-07 (the bound is 4 x that)."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import types

import numpy as np
import pytest

from tests import raft_conv_ref as R

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402
from tests.test_sep_conv_gru_cpu import make_state as make_gru_state  # noqa: E402
from tests.test_sep_conv_gru_cpu import torch_forward as gru_torch_forward  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_CLI = os.path.join(ROOT, "feature_tracker_amd", "host", "build", "raft_conv_plan_cli")
# in a directory of its own: tests/test_oracle_cpu.py replays every .npz directly under tests/golden/ through the KLT / matcher oracle
GOLDEN = os.path.join(ROOT, "tests", "golden", "raft", "raft_update_block_small.npz")

# (net, inp, corr, corr_hidden, corr_out, flow_hidden, flow_out, motion_out, mask_hidden; B, H, W): the issue's small case, odd channel
# counts everywhere, and the widths of the reference's model.py:105-117 (3 levels of radius 3: 147 correlation channels) on a 5 x 5 grid
CASES = [(16, 3, 18, 16, 12, 8, 4, 10, 8, 2, 6, 7), (13, 5, 19, 17, 11, 9, 7, 15, 21, 1, 5, 9), (64, 128, 147, 64, 32, 32, 16, 32, 64, 1, 5, 5)]
MASK_CHANNELS = 8 * 8 * 9  # update_block.py:59
GRU_KERNEL_SIZE = 5        # update_block.py:54
MEASURED_SEEDS = (1, 2, 3, 4)
FIFTH_SEED = 5
# max |restatement - float64| over CASES x MEASURED_SEEDS and the three outputs, and the asserted bound: 4 x it, for
# other seeds and the growth of a K-term chain's error with its inputs
MEASURED_MAX_ABS = 4.18e-07
BOUND = 4 * MEASURED_MAX_ABS


def layer_shapes(net, inp, corr, corr_hidden, corr_out, flow_hidden, flow_out, motion_out, mask_hidden):
    """The nine Conv2d layers of update_block.py:4-60 under the module's names: (out_channels, in_channels, kernel_size)."""
    return {"motion_encoder.correlation_conv.0": (corr_hidden, corr, 1), "motion_encoder.correlation_conv.2": (corr_out, corr_hidden, 3),
            "motion_encoder.flow_conv.0": (flow_hidden, 2, 7), "motion_encoder.flow_conv.2": (flow_out, flow_hidden, 3),
            "motion_encoder.out_conv.0": (motion_out - 2, corr_out + flow_out, 3),
            "flow_head.conv1": (flow_out, net, 3), "flow_head.conv2": (2, flow_out, 3),  # FlowHead(net, flow_out): its hidden width is flow_out (:55)
            "mask.0": (mask_hidden, net, 3), "mask.2": (MASK_CHANNELS, mask_hidden, 1)}


def make_state(widths, seed):
    """The reference module's own default initialisation: torch.nn.Conv2d layers of its shapes, seeded; the GRU's as its own test makes them."""
    net, inp, motion_out = widths[0], widths[1], widths[7]
    state = {"gru." + k: v for k, v in make_gru_state(inp + motion_out, net, GRU_KERNEL_SIZE, seed).items()}
    torch.manual_seed(100 + seed)
    for name, (M, Cin, ks) in layer_shapes(*widths).items():
        conv = torch.nn.Conv2d(Cin, M, ks, stride=1, padding=ks // 2)
        state[name + ".weight"] = conv.weight.detach().clone()
        state[name + ".bias"] = conv.bias.detach().clone()
    return state


def make_inputs(widths, B, H, W, seed):
    """net as a hidden state (tanh), inp as a context feature (relu), correlation features, a flow of a few pixels."""
    g = torch.Generator().manual_seed(2000 + seed)
    net, inp, corr = widths[:3]
    return (torch.tanh(torch.randn(B, net, H, W, generator=g)), torch.relu(torch.randn(B, inp, H, W, generator=g)), torch.randn(B, corr, H, W, generator=g),
            2.0 * torch.randn(B, 2, H, W, generator=g))


def torch_forward(state, net, inp, correlation, flow, dtype=None):
    """update_block.py:61-67 with :36-43 and :10-14, line by line, in ``dtype`` (default: that of the arguments).  Returns (new_net, mask,
    delta_flow, out): the module's three outputs and the motion encoder's ``out`` before :41's cat."""
    F = torch.nn.functional
    dtype = dtype or net.dtype
    net, inp, correlation, flow = (t.to(dtype) for t in (net, inp, correlation, flow))

    def conv(x, name):
        w = state[name + ".weight"].to(dtype)
        return F.conv2d(x, w, state[name + ".bias"].to(dtype), stride=1, padding=w.shape[-1] // 2)

    temp_correlation = F.relu(conv(F.relu(conv(correlation, "motion_encoder.correlation_conv.0")), "motion_encoder.correlation_conv.2"))
    temp_flow = F.relu(conv(F.relu(conv(flow, "motion_encoder.flow_conv.0")), "motion_encoder.flow_conv.2"))
    out = F.relu(conv(torch.cat([temp_correlation, temp_flow], dim=1), "motion_encoder.out_conv.0"))
    motion = torch.cat([out, flow], dim=1)
    inp_motion = torch.cat([inp, motion], dim=1)
    new_net = gru_torch_forward({k[4:]: v for k, v in state.items() if k.startswith("gru.")}, inp_motion, net, dtype)
    delta_flow = conv(F.relu(conv(new_net, "flow_head.conv1")), "flow_head.conv2")
    mask = .25 * conv(F.relu(conv(new_net, "mask.0")), "mask.2")
    return new_net, mask, delta_flow, out


@functools.lru_cache(maxsize=None)
def case(k, seed):
    """(state as numpy, the four inputs, the float64 reference's three outputs) of CASES[k] with ``seed``, computed once and shared;
    nobody writes to them."""
    widths, (B, H, W) = CASES[k][:9], CASES[k][9:]
    state = make_state(widths, seed)
    inputs = make_inputs(widths, B, H, W, seed)
    ref64 = tuple(t.numpy() for t in torch_forward(state, *inputs, dtype=torch.float64)[:3])
    return R.weights_of(state), tuple(t.numpy() for t in inputs), ref64


def max_abs(got, want):
    return max(float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) for a, b in zip(got, want))


@pytest.mark.parametrize("k", range(len(CASES)), ids=[str(c) for c in CASES])
def test_restatement_against_float64(k):
    worst = []
    for seed in MEASURED_SEEDS + (FIFTH_SEED,):
        state, inputs, ref64 = case(k, seed)
        worst.append(max_abs(R.update_block(*inputs, state)[:3], ref64))
    print(f"case {CASES[k]}: max |restatement - float64| per seed {['%.3g' % w for w in worst]} (measured maximum {MEASURED_MAX_ABS:.3g}, bound {BOUND:.3g})")
    assert max(worst[:-1]) <= MEASURED_MAX_ABS * 1.0001, "the recorded maximum is out of date"
    assert max(worst) <= BOUND


@pytest.mark.parametrize("name", sorted(R.MUTANTS))
def test_mutants_fail_the_float64_bound(name):
    worst = []
    for k in range(len(CASES)):
        state, inputs, ref64 = case(k, MEASURED_SEEDS[0])
        worst.append(max_abs(R.update_block(*inputs, state, variant=R.MUTANTS[name])[:3], ref64))
    print(f"mutant {name}: {['%.3g' % w for w in worst]} (bound {BOUND:.3g})")
    assert min(worst) > BOUND  # on every case, which is more than the one case that would do


# ---- the golden fixture: the reference's own module on torch CPU (tests/golden/make_raft_update_block.py) ------------------------


def golden():
    z = np.load(GOLDEN)
    state = {k[len("state/"):]: z[k] for k in z.files if k.startswith("state/")}
    return z, state


def test_golden_fixture_of_the_reference_module():
    import feature_tracker_amd as F
    assert os.path.getsize(GOLDEN) < 100 * 1000
    z, state = golden()
    widths, (B, H, W) = tuple(int(e) for e in z["sizes"][:9]), (int(e) for e in z["sizes"][9:])
    assert widths == CASES[0][:9] and (H, W) == (3, 4)
    # exactly the module's key names: ours reads every one of them and asks for no other
    assert set(state) == set(make_state(widths, 1)) and all(state[k].shape == tuple(v.shape) for k, v in make_state(widths, 1).items())
    block = F.UpdateBlock.from_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, prefix="")
    assert set(block.weights) == set(state)
    assert (block.net_channels, block.inp_channels, block.mask_channels, block.gru.kernel_size) == (16, 3, MASK_CHANNELS, GRU_KERNEL_SIZE)
    assert block.motion_encoder.layer_shapes() == {k[len("motion_encoder."):]: v for k, v in layer_shapes(*widths).items() if k.startswith("motion_encoder.")}
    whole = {"update_block." + k: torch.from_numpy(v) for k, v in state.items()}
    assert set(F.UpdateBlock.from_state_dict(whole).weights) == set(state)  # the default prefix is a whole Raft's
    got = R.update_block(z["net"], z["inp"], z["correlation"], z["flow"], R.weights_of(state))[:3]
    want = (z["new_net"], z["mask"], z["delta_flow"])
    assert [g.shape for g in got] == [w.shape for w in want] and all(w.dtype == np.float32 for w in want)
    worst = max_abs(got, want)
    print(f"restatement against the reference module's recorded float32 outputs: {worst:.3g} (bound {BOUND:.3g})")
    assert worst <= BOUND


# ---- known answers -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("ks,H,W", [(3, 1, 1), (3, 2, 1), (3, 1, 2), (3, 2, 2), (7, 1, 1), (7, 1, 7), (7, 7, 1), (7, 3, 3), (7, 2, 5), (7, 6, 4)])
def test_single_tap_shows_direction_and_zero_padding(ks, H, W):
    """One non-zero weight at (ty, tx) and a one-hot image: out[y][x] = in[y + ty - pad][x + tx - pad] (correlation, not convolution), and
    exactly +0 where the tap is outside the image.  Images smaller than the kernel: most taps never land inside."""
    pad = ks // 2
    for (ty, tx), (py, px) in itertools.product(itertools.product(range(ks), repeat=2), ((0, 0), (H - 1, W - 1), (H // 2, 0))):
        image = np.zeros((1, 1, H, W), np.float32)
        image[0, 0, py, px] = 3.0
        weight = np.zeros((1, 1, ks, ks), np.float32)
        weight[0, 0, ty, tx] = 1.0
        want = np.zeros_like(image)
        y, x = py - (ty - pad), px - (tx - pad)
        if 0 <= y < H and 0 <= x < W:
            want[0, 0, y, x] = 3.0
        got = R.conv2d(image, weight, np.zeros(1, np.float32), relu=False)
        assert R.same(got, want), (ty, tx, py, px)


def test_epilogue_order_and_special_values():
    """ReLU first, then the scale; ReLU keeps a NaN and -0 (it is not fmaxf); a tap outside the image is multiplied, not skipped: it
    turns an accumulator of -0 into +0, and with an infinite weight into NaN."""
    x = np.float32([[[[1.0, -2.0, np.nan, 0.0]]]])
    w, b = np.ones((1, 1, 1, 1), np.float32), np.zeros(1, np.float32)
    out = R.conv2d(x, w, b, relu=True, scale=0.25)[0, 0, 0]
    assert out[0] == 0.25 and out[1] == 0 and not np.signbit(out[1]) and np.isnan(out[2]) and out[3] == 0
    out = R.conv2d(x, w, b, relu=True, scale=-0.25)[0, 0, 0]
    assert out[0] == -0.25 and out[1] == 0 and np.signbit(out[1])  # scale * relu(v), not relu(scale * v)
    minus_zero = R.conv2d(np.float32([[[[0.0]]]]), w, np.float32([-0.0]), relu=True)
    assert minus_zero[0, 0, 0, 0] == 0 and not np.signbit(minus_zero[0, 0, 0, 0])  # fmaf(1, +0, -0) = +0
    minus_zero = R.conv2d(np.float32([[[[0.0]]]]), -w, np.float32([-0.0]), relu=True)
    assert np.signbit(minus_zero[0, 0, 0, 0])  # fmaf(-1, +0, -0) = -0, and ReLU keeps it
    w3 = np.zeros((1, 1, 3, 3), np.float32)
    w3[0, 0, 0, 0] = np.inf
    out = R.conv2d(np.ones((1, 1, 2, 2), np.float32), w3, b, relu=False)[0, 0]
    assert np.isnan(out[0, 0]) and np.isnan(out[0, 1]) and np.isnan(out[1, 0]) and np.isinf(out[1, 1])  # inf * (+0 padding) = NaN


def test_parts_equal_their_concatenation():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 35, 4, 5)).astype(np.float32)
    for ks in (1, 3, 7):
        w = rng.standard_normal((5, 35, ks, ks)).astype(np.float32)
        b = rng.standard_normal(5).astype(np.float32)
        whole = R.conv2d(x, w, b, relu=True)
        assert R.same(R.conv2d((x[:, :3], x[:, 3:33], x[:, 33:]), w, b, relu=True), whole)
        assert R.same(R.conv2d((x[:, :8], x[:, 8:]), w, b, relu=True), whole)


# ---- the packed layout ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("M,Cin,ks", [(40, 35, 1), (33, 11, 3), (2, 4, 3), (8, 2, 7), (70, 3, 7)])
def test_packed_layout_is_the_headers(M, Cin, ks):
    """[M][K] (torch's own k) as [tile][k-step][64], lane = 32 (k % 2) + row % 32, -0 beyond K and +0 beyond M (include/ftk.h)."""
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import raft
    torch.manual_seed(M + Cin)
    weight = torch.randn(M, Cin, ks, ks)
    K, k_steps = Cin * ks * ks, N.conv2d_k_steps(Cin, ks)
    chunk = N.FTK_CONV2D_CHUNK[ks]
    assert k_steps == -(-Cin // chunk) * chunk * ks * ks // 2 and 2 * k_steps >= K
    flat = raft._pack_conv(weight).numpy()
    assert flat.size == N.conv2d_packed_elements(M, Cin, ks)
    packed = flat.reshape(-1, k_steps, 2, 32)
    matrix = weight.numpy().reshape(M, K)
    full = packed.transpose(0, 3, 1, 2).reshape(-1, 2 * k_steps)  # [32 tiles][2 k_steps]
    assert np.array_equal(full[:M, :K], matrix)
    assert (full[:, K:] == 0).all() and np.signbit(full[:, K:]).all()
    assert (full[M:, :K] == 0).all() and not np.signbit(full[M:, :K]).any()
    if os.path.exists(N.LIB_PATH):
        e = C.c_int64()
        assert N.lib().ftk_conv2d_packed_elements(M, Cin, ks, C.byref(e)) == 0 and e.value == flat.size
        assert N.lib().ftk_conv2d_packed_elements(M, Cin, 5, C.byref(e)) == -4 and N.lib().ftk_conv2d_packed_elements(1025, Cin, ks, C.byref(e)) == -4
        assert N.lib().ftk_conv2d_packed_elements(M, 0, ks, C.byref(e)) == -1


# ---- loud failures, before any device is touched -------------------------------------------------------------------------------


def test_from_state_dict_refuses_by_key():
    import feature_tracker_amd as F
    widths = CASES[0][:9]
    state = make_state(widths, 1)
    block = F.UpdateBlock.from_state_dict(state, prefix="")
    enc = block.motion_encoder
    assert (enc.correlation_in, enc.correlation_hidden, enc.correlation_out, enc.flow_hidden, enc.flow_out, enc.out_channels) == (18, 16, 12, 8, 4, 10)
    assert (block.gru.x_channels, block.gru.h_channels, block.mask_hidden_channels) == (13, 16, 8)
    sub = {k[len("motion_encoder."):]: v for k, v in state.items() if k.startswith("motion_encoder.")}
    assert set(F.MotionEncoder.from_state_dict(sub).weights) == set(sub)
    with pytest.raises(ValueError, match=r"update_block\.motion_encoder\.correlation_conv\.0\.weight is missing"):
        F.UpdateBlock.from_state_dict(state)  # the default prefix is a whole model's
    for key, bad, match in (("mask.2.bias", None, r"mask\.2\.bias is missing"),
                            ("gru.conv_q_vertical.bias", None, r"gru\.conv_q_vertical\.bias is missing"),
                            ("flow_head.conv2.weight", None, r"flow_head\.conv2\.weight is missing"),
                            ("motion_encoder.flow_conv.2.bias", None, r"motion_encoder\.flow_conv\.2\.bias is missing"),
                            ("mask.0.weight", state["mask.0.weight"].double(), r"mask\.0\.weight must be a float32"),
                            ("flow_head.conv2.weight", torch.zeros(3, 4, 3, 3), r"flow_head\.conv2\.weight must be .*\[2, 4, 3, 3\]"),
                            ("motion_encoder.flow_conv.0.weight", torch.zeros(8, 2, 5, 5), r"motion_encoder\.flow_conv\.0\.weight must be .*\[8, 2, 7, 7\]"),
                            ("motion_encoder.out_conv.0.weight", torch.zeros(8, 17, 3, 3), r"motion_encoder\.out_conv\.0\.weight must be .*\[8, 16, 3, 3\]"),
                            ("motion_encoder.correlation_conv.2.bias", torch.zeros(13), r"motion_encoder\.correlation_conv\.2\.bias must be .*\[12\]"),
                            ("mask.2.weight", torch.zeros(576, 8, 3, 3), r"mask\.2\.weight must be .*\[576, 8, 1, 1\]"),
                            ("mask.0.weight", torch.zeros(8, 16, 3), r"mask\.0\.weight must be a 4-D tensor")):
        broken = dict(state)
        if bad is None:
            del broken[key]
        else:
            broken[key] = bad
        with pytest.raises(ValueError, match=match):
            F.UpdateBlock.from_state_dict(broken, prefix="")
    with pytest.raises(ValueError, match="out_channels 2 must be at least 3"):
        F.MotionEncoder(18, 16, 12, 8, 4, 2)
    with pytest.raises(ValueError, match="correlation_in 0"):
        F.MotionEncoder(0, 16, 12, 8, 4, 10)
    with pytest.raises(ValueError, match="above 4096 -> 1024"):
        F.MotionEncoder(18, 1025, 12, 8, 4, 10)


def test_wrappers_refuse_bad_arguments_without_a_device():
    import feature_tracker_amd as F
    widths, (B, H, W) = CASES[0][:9], CASES[0][9:]
    block = F.UpdateBlock.from_state_dict(make_state(widths, 1), prefix="")
    net, inp, corr, flow = make_inputs(widths, B, H, W, 1)
    bad = [
        ("net must be", (net.double(), inp, corr, flow)), ("inp must be", (net, inp.half(), corr, flow)), ("correlation must be", (net, inp, corr[0], flow)),
        ("flow must be", (net, inp, corr, flow.numpy())), ("flow must be .*2, H, W", (net, inp, corr, torch.zeros(B, 3, H, W))),
        ("net must be .*16, H, W", (torch.zeros(B, 17, H, W), inp, corr, flow)), ("correlation must be .*18, H, W", (net, inp, corr[:, :17], flow)),
        ("inp and net must agree", (net, torch.zeros(B, 3, H + 1, W), corr, flow)), ("flow and net must agree", (net, inp, corr, torch.zeros(B + 1, 2, H, W))),
        ("net must not be empty", (net[:, :, :0], inp[:, :, :0], corr[:, :, :0], flow[:, :, :0])),
    ]
    for match, args in bad:
        with pytest.raises(ValueError, match=match):
            block(*args)
    for k in range(4):
        args = [net, inp, corr, flow]
        args[k] = args[k].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match="UpdateBlock is inference only"):
            block(*args)
        with torch.no_grad(), pytest.raises(ValueError, match="no CPU fallback"):
            block(*args)
    with pytest.raises(ValueError, match="no CPU fallback"):
        block(net, inp, corr, flow)
    enc = block.motion_encoder
    for match, args in (("correlation must be", (corr.double(), flow)), ("flow must be", (corr, flow[:, :1])), ("flow and correlation must agree", (corr, flow[:, :, :, :3]))):
        for entry in (enc.features, enc):
            with pytest.raises(ValueError, match=match):
                entry(*args)
    for entry in (enc.features, enc):
        with pytest.raises(RuntimeError, match="MotionEncoder is inference only"):
            entry(corr, flow.clone().requires_grad_(True))
        with pytest.raises(ValueError, match="no CPU fallback"):
            entry(corr, flow)
    with pytest.raises(ValueError, match="no weights yet"):
        F.MotionEncoder(18, 16, 12, 8, 4, 10).features(corr, flow)


def test_device_entry_refuses_bad_arguments_without_a_device():
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    ctx = types.SimpleNamespace(handle=None)
    x, out = torch.zeros(1, 3, 3, 5), torch.zeros(1, 4, 3, 5)
    w, b = torch.zeros(N.conv2d_packed_elements(4, 3, 3)), torch.zeros(4)
    with pytest.raises(ValueError, match="^out must be a CUDA tensor"):
        D.conv2d_device(ctx, [x], w, b, 3, True, 1.0, out)
    with pytest.raises(ValueError, match="^out must be .*wrong dtype"):
        D.conv2d_device(ctx, [x], w, b, 3, True, 1.0, out.double())
    with pytest.raises(ValueError, match="kernel_size 5"):
        D.conv2d_device(ctx, [x], w, b, 5, True, 1.0, out)
    with pytest.raises(ValueError, match="1 .. 3 tensors"):
        D.conv2d_device(ctx, [x] * 4, w, b, 3, True, 1.0, out)
    with pytest.raises(ValueError, match="out_scale must be finite"):
        D.conv2d_device(ctx, [x], w, b, 3, True, float("nan"), out)


# the walk of tests/args_walk.py (duck-typed tensors, a recording stand-in for the native library) over this entry
WALK_TENSORS = 1 + 3 + 2  # out, three parts, the packed weights and the bias


def _walk_call(w):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    B, H, W, M, ks = 2, 3, 7, 40, 3
    out = w.t("out", "float32", B, M, H, W)
    parts = [w.t(f"parts[{i}]", "float32", B, c, H, W) for i, c in enumerate((3, 30, 2))]
    weights = w.t("packed_weights", "float32", N.conv2d_packed_elements(M, 35, ks))
    bias = w.t("bias", "float32", M)
    return D.conv2d_device(w.ctx, parts, weights, bias, ks, True, 0.25, out)


def test_device_entry_takes_no_pointer_of_an_unchecked_argument(monkeypatch):
    w = A.walk_call(monkeypatch, _walk_call, ["ftk_conv2d_device"])
    assert len(w.made) == WALK_TENSORS


@pytest.mark.parametrize("which", range(WALK_TENSORS))
@pytest.mark.parametrize("kind", ["dtype", "shape", "device"])
def test_device_entry_stops_before_the_library(monkeypatch, which, kind):
    """Each tensor of the call in turn made float64, one element longer in its last dimension, or moved to another device."""
    w = A.Walk(monkeypatch, spoil=(which, kind, A.one_column_more if kind == "shape" else None))
    with pytest.raises(ValueError) as e:
        _walk_call(w)
    name = w.spoiled.name
    if not (kind == "shape" and name == "out"):  # a wider out is a legal out: the first part is then the one refused
        assert name in str(e.value), (name, str(e.value))
    assert w.lib.calls == [] and w.unchecked_reads == []


# ---- the launch plan -----------------------------------------------------------------------------------------------------------

LDS_LIMIT = 64 * 1024
PLAN_FIELDS = ("out_channels", "in_channels", "kernel_size", "B", "H", "W")


def plan(cases):
    assert os.path.exists(PLAN_CLI), "host layer not built (python -c 'import __graft_entry__ as g; g.build()')"
    text = "\n".join(" ".join(str(c[f]) for f in PLAN_FIELDS) for c in cases) + "\n"
    r = subprocess.run([PLAN_CLI], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        d = {}
        for kv in line.split():
            k, v = kv.split("=")
            d[k] = tuple(int(e) for e in v.split("x")) if k in ("grid", "block") else int(v) if v.lstrip("-").isdigit() else v
        out.append(d)
    assert len(out) == len(cases)
    return out


def cdiv(a, b):
    return -(-a // b)


def test_plan_properties():
    from feature_tracker_amd import _native as N
    cases = []
    for (M, Cin), ks, (B, H, W) in itertools.product(
            ((1, 1), (2, 64), (16, 18), (33, 3), (64, 131), (96, 2), (128, 256), (256, 324), (576, 256), (1024, 4096)), (1, 3, 7),
            ((1, 1, 1), (2, 6, 7), (1, 1, 7), (1, 7, 1), (1, 3, 3), (1, 5, 131), (1, 55, 128), (3, 33, 129), (1, 1, 100000), (1, 100000, 1))):
        cases.append(dict(out_channels=M, in_channels=Cin, kernel_size=ks, B=B, H=H, W=W))
    seen_wm = set()
    for c, p in zip(cases, plan(cases)):
        what = f"{c} -> {p}"
        assert p["refused"] == "none", what
        M, ks = c["out_channels"], c["kernel_size"]
        pad = ks // 2
        seen_wm.add(p["wm"])
        assert p["m_tiles"] == cdiv(M, 32) and p["wm"] * p["wn"] == 4 and p["wm"] in (1, 2, 4), what
        # every output channel and pixel belongs to exactly one (workgroup, wave, MFMA tile): the row tiles of the workgroups along y
        # partition the channel tiles, their pixel tiles partition the image, tile after tile without overlap
        assert p["m_groups"] == cdiv(p["m_tiles"], p["wm"]) and (p["m_groups"] - 1) * p["wm"] < p["m_tiles"], what
        assert (p["tile_w"], p["tile_h"]) == (32, p["wn"]), what
        assert p["tiles_x"] * p["tile_w"] >= c["W"] > (p["tiles_x"] - 1) * p["tile_w"], what
        assert p["tiles_y"] * p["tile_h"] >= c["H"] > (p["tiles_y"] - 1) * p["tile_h"], what
        assert p["grid"] == (p["tiles_x"] * p["tiles_y"] * c["B"], p["m_groups"]) and p["block"] == (256, 1), what
        assert p["grid"][0] < 2 ** 31 and p["grid"][1] <= 65535, what
        # the chunks cover every k in order, in whole k-steps, and agree with the Python packer
        chunk = N.FTK_CONV2D_CHUNK[ks]
        assert p["chunk"] == chunk and p["chunks"] == cdiv(c["in_channels"], chunk) and p["steps_per_chunk"] * 2 == chunk * ks * ks, what
        assert p["k_steps"] == p["chunks"] * p["steps_per_chunk"] == N.conv2d_k_steps(c["in_channels"], ks) and 2 * p["k_steps"] >= c["in_channels"] * ks * ks, what
        assert p["packed"] == p["m_tiles"] * p["k_steps"] * 64 == N.conv2d_packed_elements(M, c["in_channels"], ks), what
        # LDS: per staged channel wn + 2 pad rows of 32 + 2 pad floats, inside the kernel's static array, inside 64 KiB
        strip = (p["wn"] + 2 * pad) * (32 + 2 * pad)
        assert p["pitch"] == strip and p["lds"] == chunk * strip * 4 <= p["lds_static"] <= LDS_LIMIT, what
        assert p["lds_static"] == chunk * (4 + 2 * pad) * (32 + 2 * pad) * 4, what
        assert p["mfma"] == "32x32x2_f32", what
    assert seen_wm == {1, 2, 4}


def test_plan_refuses_limits_by_name():
    base = dict(out_channels=16, in_channels=19, kernel_size=3, B=1, H=4, W=4)
    cases = [dict(base, kernel_size=5), dict(base, kernel_size=0), dict(base, kernel_size=9), dict(base, out_channels=0), dict(base, out_channels=1025),
             dict(base, in_channels=0), dict(base, in_channels=4097), dict(base, B=0), dict(base, W=0), dict(base, H=-1),
             dict(base, B=2 ** 31 - 1, H=2 ** 31 - 1), dict(base, W=2 ** 31 - 1, H=2 ** 31 - 1), dict(base, out_channels=1024, in_channels=4096), dict(base, kernel_size=7, out_channels=1, in_channels=1)]
    got = [p["refused"] for p in plan(cases)]
    assert got == ["kernel_size", "kernel_size", "kernel_size", "out_channels", "out_channels", "in_channels", "in_channels", "sizes", "sizes", "sizes", "grid",
                   "grid", "none", "none"]
