"""SuperPoint without a device: the launch plan of conv2d_kernel's pooled form through its command-line tool, and every
earlier case of that tool answered as the parent commit answered it (tests/golden/superpoint/raft_conv_plan_recorded.txt); the scalar
restatement (tests/superpoint_ref.c) against torch on the CPU: its pool bit for bit against torch.max_pool2d, the whole network against
the float64 composition of the same ops; the mutants of the restatement; and the walk of the Python entries over recording stand-ins.

Measured (printed by the tests, -s shows them): restatement against float64 over NETWORK_CASES x MEASURED_SEEDS, the largest absolute
difference of the two head tensors: 1.22e-07 (the bound is 4 x that)."""
import functools
import os
import subprocess
import types

import numpy as np
import pytest

from tests import superpoint_ref as R

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_CLI = os.path.join(ROOT, "feature_tracker_amd", "host", "build", "raft_conv_plan_cli")
RECORDED = os.path.join(ROOT, "tests", "golden", "superpoint", "raft_conv_plan_recorded.txt")

# (c1, c2, c3, c4, head, D; H, W): narrow widths at one cell, at several cells and at more than one 32-pixel tile, and upstream's widths
NARROW, UPSTREAM = (4, 4, 8, 8, 8, 16), (64, 64, 128, 128, 256, 256)
NETWORK_CASES = [(NARROW, 8, 8), (NARROW, 16, 24), (NARROW, 40, 72), (UPSTREAM, 16, 24)]
MEASURED_SEEDS = (1, 2, 3)
EXTRA_SEED = 4
# max |restatement - float64| over NETWORK_CASES x MEASURED_SEEDS and both head tensors, and the asserted bound: 4 x it,
# for other seeds of the same distribution
MEASURED_DEVIATION = 1.22e-07
BOUND = 4 * MEASURED_DEVIATION

# the pooled layer: (kernel size, relu, channels of the parts, out_channels, H, W, B).  Together: both kernel sizes with and without ReLU;
# C_in 1, 8, 9, 20 (below, at and above one chunk of 8, two chunks with a tail); out_channels 1, 32, 33, 64, 65, 130 (wm 1 / wn 4 and wm 2 /
# wn 2, an idle channel tail, m_groups > 1); 2 x 2, 3 x 3, 5 x 70, 9 x 33, 8 x 64 (odd sizes dropped, a tile edge next to a pooling pair, a
# last workgroup with fewer rows than wn); B 1 and 2; one and two parts
POOL_CASES = [(3, True, (1,), 1, 2, 2, 1), (3, False, (8,), 32, 3, 3, 2), (1, True, (9,), 33, 5, 70, 1), (3, True, (12, 8), 64, 9, 33, 2),
              (1, False, (20,), 65, 8, 64, 1), (3, False, (5, 4), 130, 5, 70, 1), (3, True, (8,), 65, 9, 33, 1), (1, True, (1,), 130, 3, 3, 2),
              (3, True, (20,), 33, 8, 64, 1), (1, False, (4, 4), 32, 2, 2, 2)]
NORMALISE_CHANNELS = (1, 63, 64, 65, 256)
NORMALISE_GRIDS = ((1, 1), (3, 5), (9, 33))


@functools.lru_cache(maxsize=None)
def pool_case(k):
    """(parts, weight, bias) of POOL_CASES[k], seeded; nobody writes to them."""
    ks, _, channels, M, H, W, B = POOL_CASES[k]
    rng = np.random.default_rng(500 + k)
    parts = tuple(rng.standard_normal((B, c, H, W)).astype(np.float32) for c in channels)
    weight = (rng.standard_normal((M, sum(channels), ks, ks)) / np.sqrt(sum(channels) * ks * ks)).astype(np.float32)
    bias = rng.standard_normal(M).astype(np.float32)
    for a in parts + (weight, bias):
        a.setflags(write=False)
    return parts, weight, bias


def hostile_pool_layer():
    """A 1 x 1 layer that hands the hostile image on bit for bit (fmaf(1, x, -0) = x, the sign of a zero included) in its first output
    channel and negated in its second."""
    image = R.hostile_pool_image()
    return image[None, None], np.float32([1.0, -1.0]).reshape(2, 1, 1, 1), np.float32([-0.0, -0.0])


@functools.lru_cache(maxsize=None)
def normalise_case(d, hc, wc):
    """A descriptor map with, where there is room, an all-zero cell, a cell with a NaN and a cell whose squares underflow."""
    x = np.random.default_rng(600 + d + hc).standard_normal((d, hc, wc)).astype(np.float32)
    if hc * wc > 1:
        x[:, 0, 0] = 0.0
        x[d // 2, hc - 1, wc - 1] = np.nan
        x[:, hc - 1, 0] = np.float32(1e-30)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def network_case(k, seed):
    """(state as float32 arrays, image) of NETWORK_CASES[k] with ``seed``."""
    widths, H, W = NETWORK_CASES[k]
    return R.weights_of(R.make_state(widths, seed)), R.make_image(H, W, seed)


@functools.lru_cache(maxsize=None)
def network_heads(k, seed):
    """The restatement's heads of that case, computed once and shared between the tests of this file and the GPU tests."""
    state, image = network_case(k, seed)
    semi, desc = R.heads(image, state)
    semi.setflags(write=False)
    return semi, desc


def float64_heads(state, image):
    """Upstream's forward pass in stock torch ops, float64."""
    F = torch.nn.functional
    g = lambda k: torch.from_numpy(state[k]).double()  # noqa: E731
    conv = lambda x, name: F.conv2d(x, g(name + ".weight"), g(name + ".bias"), padding=state[name + ".weight"].shape[-1] // 2)  # noqa: E731
    x = torch.from_numpy(image).double()[None, None]
    for name in R.LAYERS[:8]:
        x = F.relu(conv(x, name))
        if name in R.POOLED:
            x = F.max_pool2d(x, 2, 2)
    semi = conv(F.relu(conv(x, "convPa")), "convPb")
    desc = F.normalize(conv(F.relu(conv(x, "convDa")), "convDb"), p=2, dim=1)
    return semi[0].numpy(), desc[0].numpy()


def max_abs(got, want):
    return max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(got, want))


# ---- the launch plan -----------------------------------------------------------------------------------------------------------


def run_plan(lines):
    assert os.path.exists(PLAN_CLI), "host layer not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([PLAN_CLI], input="".join(line + "\n" for line in lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def parse(line):
    d = {}
    for kv in line.split():
        k, v = kv.split("=")
        d[k] = tuple(int(e) for e in v.split("x")) if k in ("grid", "block") else int(v) if v.lstrip("-").isdigit() else v
    return d


def test_every_earlier_plan_case_is_answered_as_before():
    """The cases of tests/test_update_block_cpu.py and tests/test_raft_encoder_cpu.py, with the tool's answers recorded on the parent commit."""
    with open(RECORDED) as f:
        recorded = [line.rstrip("\n").split("|") for line in f if line.strip()]
    assert len(recorded) == 453
    got = run_plan([case for case, _ in recorded])
    assert [g for g, (_, want) in zip(got, recorded) if g != want] == []


def test_pooled_plan_properties():
    cases = [(M, Cin, ks, B, H, W) for M in (1, 32, 33, 64, 65, 96, 128, 130, 1024) for Cin, ks in ((1, 3), (20, 3), (64, 1))
             for B, H, W in ((1, 2, 2), (2, 3, 3), (1, 5, 70), (1, 9, 33), (1, 8, 64), (1, 480, 752), (1, 2, 100001))]
    plain = [parse(line) for line in run_plan([" ".join(str(e) for e in c) + " 1" for c in cases])]
    pooled = [parse(line) for line in run_plan([" ".join(str(e) for e in c) + " 1 1" for c in cases])]
    seen = set()
    for (M, Cin, ks, B, H, W), p, q in zip(cases, pooled, plain):
        what = f"{(M, Cin, ks, B, H, W)} -> {p}"
        assert p["refused"] == "none" and p["pool"] == 1 and "pool" not in q, what
        seen.add((p["wm"], p["wn"]))
        # an even number of rows per workgroup, whatever the channel count; the channel tiles still partition into the groups
        assert p["wm"] == min(p["m_tiles"], 2) and p["wn"] == 4 // p["wm"] and p["wn"] % 2 == 0 and p["m_tiles"] == -(-M // 32), what
        assert p["m_groups"] == -(-p["m_tiles"] // p["wm"]) and (p["m_groups"] - 1) * p["wm"] < p["m_tiles"], what
        # floored sizes; the tiles are of convolution pixels and cover exactly the rows and columns a window reads
        assert (p["out_h"], p["out_w"], p["stride"]) == (H // 2, W // 2, 1), what
        assert (p["tile_w"], p["tile_h"]) == (32, p["wn"]), what
        assert p["tiles_x"] * 32 >= 2 * (W // 2) > (p["tiles_x"] - 1) * 32 and p["tiles_y"] * p["wn"] >= 2 * (H // 2) > (p["tiles_y"] - 1) * p["wn"], what
        assert p["grid"] == (p["tiles_x"] * p["tiles_y"] * B, p["m_groups"]) and p["block"] == (256, 1), what
        # the chunks, the packed weights and a staged row are the unpooled plan's; the hand-off of 2 x 16 x 32 floats fits the static array
        for key in ("chunk", "chunks", "steps_per_chunk", "k_steps", "packed", "row", "lds_static", "mfma"):
            assert p[key] == q[key], (key, what)
        assert p["rows"] == p["wn"] + 2 * (ks // 2) and p["pitch"] == p["rows"] * p["row"] and p["lds"] == p["chunk"] * p["pitch"] * 4 <= p["lds_static"], what
        assert 2 * 16 * 32 * 4 <= p["lds_static"], what
    assert seen == {(1, 4), (2, 2)}


def test_pooled_plan_refusals():
    base = (16, 19, 3, 1, 4, 4)
    line = lambda c, stride=1, pool=1: " ".join(str(e) for e in c) + f" {stride} {pool}"  # noqa: E731
    cases = [line(base), line(base, stride=2), line((16, 19, 7, 1, 4, 4)), line((16, 19, 3, 1, 1, 4)), line((16, 19, 3, 1, 4, 1)), line(base, pool=2),
             line(base, pool=-1), line((16, 19, 1, 1, 2, 2)), line((16, 19, 7, 1, 4, 4), pool=0), line((16, 19, 3, 1, 1, 1), pool=0), line((1025, 19, 3, 1, 4, 4)),
             line((16, 19, 5, 1, 4, 4))]
    got = [parse(p)["refused"] for p in run_plan(cases)]
    assert got == ["none", "stride", "kernel_size", "sizes", "sizes", "pool", "pool", "none", "none", "none", "out_channels", "kernel_size"]


# ---- the restatement against torch on the CPU ------------------------------------------------------------------------------------


@pytest.mark.parametrize("k", range(len(POOL_CASES)), ids=[str(c) for c in POOL_CASES])
def test_pool_of_the_restatement_is_torchs_max_pool(k):
    """On the restatement's own tensor before the pool, with a NaN, +-inf and +-0 planted in it."""
    ks, relu, _, M, H, W, B = POOL_CASES[k]
    parts, weight, bias = pool_case(k)
    out, pre = R.conv2d_pool(parts, weight, bias, relu, return_pre=True)
    assert out.shape == (B, M, H // 2, W // 2) and R.same(pre, R.raft_conv_ref.conv2d(parts, weight, bias, relu))
    assert R.same(out, torch.max_pool2d(torch.from_numpy(pre), 2, 2).numpy())
    planted = pre.copy()
    flat = planted.reshape(-1)
    for i, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, -0.0, 0.0)):
        flat[(7 * i + 3 * k) % flat.size] = v
    assert R.same(R.max_pool(planted), torch.max_pool2d(torch.from_numpy(planted), 2, 2).numpy())


def test_pool_of_hostile_values_is_torchs_max_pool():
    x, weight, bias = hostile_pool_layer()
    out, pre = R.conv2d_pool(x, weight, bias, False, return_pre=True)
    assert R.same(pre[0, 0], x[0, 0]) and R.same(pre[0, 1], -x[0, 0])
    want = torch.max_pool2d(torch.from_numpy(pre), 2, 2).numpy()
    assert R.same(out, want)
    got = out[0, 0].reshape(-1)
    assert np.isnan(got[:4]).all() and np.isposinf(got[4:8]).all() and (got[8:12] == np.float32(-3.5)).all()
    assert np.signbit(got[12:16]).tolist() == [True, False, False, False] and np.signbit(got[16:20]).tolist() == [False, True, True, True]
    assert (got[20:24] == np.float32(1e-45)).all()
    assert np.signbit(R.conv2d_pool(x, weight, bias, True)[0, 0].reshape(-1)[12:16]).tolist() == [True, False, False, False]  # the ReLU keeps -0


@pytest.mark.parametrize("d", NORMALISE_CHANNELS)
@pytest.mark.parametrize("grid", NORMALISE_GRIDS, ids=str)
def test_normalisation_of_the_restatement_against_torch(d, grid):
    x = normalise_case(d, *grid)
    y = R.channel_normalise(x)
    assert y.shape == grid + (d,)
    want = torch.nn.functional.normalize(torch.from_numpy(x.copy()).double()[None], p=2, dim=1)[0].permute(1, 2, 0).numpy()
    ok = np.isfinite(want).all(axis=2) & ~np.isnan(x).any(axis=0)
    assert np.abs(y[ok].astype(np.float64) - want[ok]).max() <= 2.0 ** -22  # two roundings of values below 1 and the chain's error
    if grid != (1, 1):
        assert (y[0, 0] == 0).all() and np.isnan(y[-1, -1, d // 2])  # 0 / 1e-12 = 0; a NaN stays where it was
        assert (y[-1, 0] == np.float32(1e-30) / np.float32(1e-12)).all()  # the squares underflow: the floor divides


@pytest.mark.parametrize("k", range(len(NETWORK_CASES)), ids=[str(c) for c in NETWORK_CASES])
def test_network_against_float64(k):
    worst = []
    for seed in MEASURED_SEEDS + (EXTRA_SEED,):
        state, image = network_case(k, seed)
        got = network_heads(k, seed) if seed == MEASURED_SEEDS[0] else R.heads(image, state)
        want = float64_heads(state, image)
        assert got[0].shape == want[0].shape == (65, image.shape[0] // 8, image.shape[1] // 8) and got[1].shape == want[1].shape
        worst.append(max_abs(got, want))
    print(f"case {NETWORK_CASES[k]}: max |restatement - float64| per seed {['%.3g' % w for w in worst]} (measured maximum {MEASURED_DEVIATION:.3g}, bound "
          f"{BOUND:.3g})")
    assert max(worst[:-1]) <= MEASURED_DEVIATION * 1.0001, "the recorded maximum is out of date"
    assert max(worst) <= BOUND


@pytest.mark.parametrize("name", sorted(R.MUTANTS))
def test_mutants_differ_from_the_restatement(name):
    variant = R.MUTANTS[name]
    differs = []
    for k in range(len(NETWORK_CASES) - 1):  # the narrow cases
        state, image = network_case(k, MEASURED_SEEDS[0])
        got = R.heads(image, state, variant)
        differs.append(not all(R.same(a, b) for a, b in zip(got, network_heads(k, MEASURED_SEEDS[0]))))
    x, weight, bias = hostile_pool_layer()
    differs.append(not R.same(R.conv2d_pool(x, weight, bias, False, variant), R.conv2d_pool(x, weight, bias, False)))
    zero_cell = normalise_case(64, 3, 5)
    differs.append(not R.same(R.channel_normalise(zero_cell, variant), R.channel_normalise(zero_cell)))
    print(f"mutant {name}: differs on {differs}")
    assert any(differs)
    if variant in (R.MUTANT_POOL_SHIFTED, R.MUTANT_HEADS_EXCHANGED):  # these two also leave the float64 bound, on every narrow case
        for k in range(len(NETWORK_CASES) - 1):
            state, image = network_case(k, MEASURED_SEEDS[0])
            assert max_abs(R.heads(image, state, variant), float64_heads(state, image)) > BOUND


# ---- the Python entries over recording stand-ins -----------------------------------------------------------------------------------


def _pool_call(w, ks=3, H=5, W=7):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    B, M = 2, 40
    out = w.t("out", "float32", B, M, H // 2, W // 2)
    parts = [w.t(f"parts[{i}]", "float32", B, c, H, W) for i, c in enumerate((3, 30, 2))]
    return D.conv2d_pool_device(w.ctx, parts, w.t("packed_weights", "float32", N.conv2d_packed_elements(M, 35, ks if ks in (1, 3, 7) else 3)), w.t("bias", "float32", M), ks, True, out)


def _normalise_call(w, d=65, hc=3, wc=5, out_shape=None):
    from feature_tracker_amd import device as D
    return D.channel_normalise_device(w.ctx, w.t("x", "float32", d, hc, wc), w.t("out", "float32", *(out_shape or (hc, wc, d))))


@pytest.mark.parametrize("call,native,tensors", [(_pool_call, "ftk_conv2d_pool_device", 6), (_normalise_call, "ftk_channel_normalise_device", 2)])
def test_device_entries_take_no_pointer_of_an_unchecked_argument(monkeypatch, call, native, tensors):
    w = A.walk_call(monkeypatch, call, [native])
    assert len(w.made) == tensors
    for which in range(tensors):
        for kind in ("dtype", "shape", "device"):
            w = A.Walk(monkeypatch, spoil=(which, kind, A.one_column_more if kind == "shape" else None))
            with pytest.raises(ValueError):
                call(w)
            assert w.lib.calls == [] and w.unchecked_reads == [], (which, kind)


def test_device_entries_refuse_before_the_library(monkeypatch):
    w = A.Walk(monkeypatch)
    for match, call, kw in (("kernel_size 7 is not supported with the max-pool", _pool_call, dict(ks=7)), ("kernel_size 5", _pool_call, dict(ks=5)),
                            ("out must be .*0, 3", _pool_call, dict(H=1)), ("FTK_KEYPOINT_DECODE_MAX_CHANNELS", _normalise_call, dict(d=1025)),
                            ("non-empty", _normalise_call, dict(hc=0)), ("out must be", _normalise_call, dict(out_shape=(65, 3, 5)))):
        with pytest.raises(ValueError, match=match):
            call(w, **kw)
    assert w.lib.calls == [] and w.unchecked_reads == []


def test_a_forward_pass_is_twelve_calls_in_order(monkeypatch):
    import feature_tracker_amd as F
    sp = F.SuperPoint.from_state_dict(R.make_state(NARROW, 1))
    assert sp.widths == dict(zip(R.LAYERS, (4, 4, 4, 4, 8, 8, 8, 8, 8, 65, 8, 16))) and (sp.detector_hidden, sp.descriptor_hidden, sp.descriptor_channels) == (8, 8, 16)
    assert set(sp.weights) == {f"{layer}.{kind}" for layer in R.LAYERS for kind in ("weight", "bias")}
    # each layer packed once, convPa and convDa as one layer of their stacked output channels
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import raft
    assert set(sp._layers) == set(R.LAYERS[:8]) | {"convPa+convDa", "convPb", "convDb"}
    stacked = sp._layers["convPa+convDa"]
    assert stacked[3] == 16 and stacked[0].numel() == N.conv2d_packed_elements(16, 8, 3)
    assert torch.equal(stacked[0], raft._pack_conv(torch.cat([sp.weights["convPa.weight"], sp.weights["convDa.weight"]])))
    assert torch.equal(stacked[1], torch.cat([sp.weights["convPa.bias"], sp.weights["convDa.bias"]]))
    H, W = 16, 24
    shapes = sp.buffer_shapes(H, W)
    assert list(shapes) == list(R.LAYERS[:8]) + ["convPa+convDa", "convPb", "convDb", "desc"]
    assert shapes["conv1a"] == (1, 4, 16, 24) and shapes["conv1b"] == (1, 4, 8, 12) and shapes["conv3b"] == shapes["conv4b"] == (1, 8, 2, 3)
    assert shapes["convPa+convDa"] == (1, 16, 2, 3) and shapes["convPb"] == (1, 65, 2, 3) and shapes["convDb"] == (1, 16, 2, 3) and shapes["desc"] == (2, 3, 16)
    # the pass itself, over stand-ins of every tensor it touches
    w = A.Walk(monkeypatch)
    sp._layers = {name: (w.t(name + ".packed", "float32", int(layer[0].numel())), w.t(name + ".bias", "float32", layer[3]), layer[2], layer[3])
                  for name, layer in sp._layers.items()}
    bufs = {name: w.t(name, "float32", *shape) for name, shape in shapes.items()}
    bufs["convPa"], bufs["convDa"], bufs["convDb[0]"] = w.t("convPa", "float32", 1, 8, 2, 3), w.t("convDa", "float32", 1, 8, 2, 3), w.t("convDb[0]", "float32", 16, 2, 3)
    sp._forward(w.ctx, w.t("image", "float32", 1, 1, H, W), bufs)
    pooled = ["ftk_conv2d_device", "ftk_conv2d_pool_device"]
    assert w.lib.calls == pooled * 3 + ["ftk_conv2d_device"] * 5 + ["ftk_channel_normalise_device"] and len(w.lib.calls) == 12 == F.superpoint.LAUNCHES
    assert w.unchecked_reads == []


def test_superpoint_refuses_by_key_and_before_any_call(monkeypatch):
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    recorder = A.RecorderLib()
    monkeypatch.setattr(N, "lib", lambda: recorder)
    state = R.make_state(NARROW, 1)
    assert F.SuperPoint.from_state_dict({"net." + k: v for k, v in state.items()}, prefix="net.").widths["convDb"] == 16
    for key, bad, match in (("conv3a.weight", None, r"conv3a\.weight is missing"), ("convDb.bias", None, r"convDb\.bias is missing"),
                            ("conv1a.weight", torch.zeros(4, 3, 3, 3), r"conv1a\.weight must be .*\[out_channels, 1, 3, 3\]"),
                            ("conv2b.weight", torch.zeros(4, 4, 1, 1), r"conv2b\.weight must be .*\[out_channels, 4, 3, 3\]"),
                            ("conv4a.weight", torch.zeros(8, 8, 3), r"conv4a\.weight must be a 4-D tensor"),
                            ("conv4b.bias", torch.zeros(9), r"conv4b\.bias must be .*\[8\]"),
                            ("convPa.weight", state["convPa.weight"].double(), r"convPa\.weight must be a float32"),
                            ("convDa.weight", torch.zeros(8, 4, 3, 3), r"convDa\.weight must be .*\[out_channels, 8, 3, 3\]"),
                            ("convPb.weight", torch.zeros(64, 8, 1, 1), r"convPb\.weight must have 65 output channels"),
                            ("convDb.weight", torch.zeros(1025, 8, 1, 1), r"convDb\.weight: .*outside the supported sizes"),
                            ("conv1a.weight", torch.zeros(1025, 1, 3, 3), r"conv1a\.weight: .*outside the supported sizes")):
        broken = dict(state)
        if bad is None:
            del broken[key]
        else:
            broken[key] = bad
        with pytest.raises(ValueError, match=match):
            F.SuperPoint.from_state_dict(broken)
    wide = R.make_state((4, 4, 8, 8, 600, 16), 1)
    with pytest.raises(ValueError, match=r"convDa\.weight: convPa and convDa run as one layer of 600 \+ 600"):
        F.SuperPoint.from_state_dict(wide)
    with pytest.raises(ValueError, match="context_on_stream"):
        F.SuperPoint.from_state_dict(state, ctx=types.SimpleNamespace(handle=None))
    sp = F.SuperPoint.from_state_dict(state)
    image = torch.zeros(16, 24)
    for match, bad in (("image must be a float32", image.double()), ("image must be a float32", torch.zeros(2, 1, 16, 24)), ("image must be a float32", torch.zeros(1, 16, 24)),
                       ("image must be a float32", image.numpy()), ("multiple of 8", torch.zeros(16, 20)), ("multiple of 8", torch.zeros(0, 24)),
                       ("multiple of 8", torch.zeros(1, 1, 4, 8)), ("must be contiguous", torch.zeros(24, 16).t()), ("no CPU fallback", image),
                       ("no CPU fallback", torch.zeros(1, 1, 16, 24))):
        with pytest.raises(ValueError, match=match):
            sp.heads(bad)
        with pytest.raises(ValueError, match=match):
            sp.detect(bad, F.KeypointDecoder())
    with pytest.raises(RuntimeError, match="SuperPoint is inference only"):
        sp.heads(image.clone().requires_grad_(True))
    assert recorder.calls == []
    assert "SuperPoint" in F.__all__
