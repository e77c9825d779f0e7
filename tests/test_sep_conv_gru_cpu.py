"""RAFT's separable ConvGRU without a device: the scalar restatement (tests/sep_conv_gru_ref.c) pinned against an
independent float64 composition of gru.py:59-76 (torch.nn.functional.conv2d in float64, written out below), five mutants of the
restatement that the same bound must reject, known answers that need no float64 side, the accuracy of sigmoid_c and tanh_c against
float64, the loud failures of the Python entries before any device is touched, and the launch plan through its command-line tool.

Measured (printed by the tests, -s shows them): restatement against float64 over CASES x MEASURED_SEEDS: 6.62e-07 (the bound is 4 x
that); sigmoid_c 2.41 ulp and tanh_c 2.99 ulp of the float64 value."""
import functools
import itertools
import os
import subprocess
import types

import numpy as np
import pytest

from tests import sep_conv_gru_ref as R

torch = pytest.importorskip("torch")

from tests import args_walk as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_CLI = os.path.join(ROOT, "feature_tracker_amd", "host", "build", "sep_conv_gru_plan_cli")

# (x_channels, h_channels, kernel_size, B, H, W)
CASES = [(3, 16, 5, 2, 6, 7), (131, 40, 5, 1, 3, 9), (160, 64, 3, 1, 5, 5)]
MEASURED_SEEDS = (1, 2, 3, 4)
FIFTH_SEED = 5
# max |restatement - float64| over CASES x MEASURED_SEEDS, and the asserted bound: 4 x it, for other seeds and the
# growth of a K-term chain's error with its inputs
MEASURED_MAX_ABS = 6.62e-07
BOUND = 4 * MEASURED_MAX_ABS
# measured maxima of the sweeps below, in ulp of the float64 value; the tests assert each plus 1 ulp
SIGMOID_C_ULP, TANH_C_ULP = 2.41, 2.99


def make_state(x_channels, h_channels, ks, seed):
    """The reference module's own default initialisation: six torch.nn.Conv2d layers of its shapes (gru.py:51-56), seeded."""
    torch.manual_seed(seed)
    pad = ks // 2
    state = {}
    for d, size, padding in (("horizontal", (1, ks), (0, pad)), ("vertical", (ks, 1), (pad, 0))):
        for g in "zrq":
            conv = torch.nn.Conv2d(x_channels + h_channels, h_channels, size, stride=1, padding=padding)
            state[f"conv_{g}_{d}.weight"] = conv.weight.detach().clone()
            state[f"conv_{g}_{d}.bias"] = conv.bias.detach().clone()
    return state


def make_inputs(x_channels, h_channels, B, H, W, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(B, x_channels, H, W, generator=g), torch.randn(B, h_channels, H, W, generator=g)


def torch_forward(state, x, h, dtype=None):
    """gru.py:59-76, line by line, in ``dtype`` (default: that of the arguments)."""
    F = torch.nn.functional
    dtype = dtype or h.dtype
    x, h = x.to(dtype), h.to(dtype)
    ks = state["conv_z_horizontal.weight"].shape[3]
    for d, padding in (("horizontal", (0, ks // 2)), ("vertical", (ks // 2, 0))):
        w = {g: state[f"conv_{g}_{d}.weight"].to(dtype) for g in "zrq"}
        b = {g: state[f"conv_{g}_{d}.bias"].to(dtype) for g in "zrq"}
        xh = torch.cat([x, h], dim=1)
        z = torch.sigmoid(F.conv2d(xh, w["z"], b["z"], padding=padding))
        r = torch.sigmoid(F.conv2d(xh, w["r"], b["r"], padding=padding))
        q = torch.tanh(F.conv2d(torch.cat([x, r * h], dim=1), w["q"], b["q"], padding=padding))
        h = (1 - z) * h + z * q
    return h


@functools.lru_cache(maxsize=None)
def case(k, seed):
    """(state as numpy, x, h, float64 reference) of CASES[k] with ``seed``, computed once and shared; nobody writes to them."""
    Cx, Ch, ks, B, H, W = CASES[k]
    state = make_state(Cx, Ch, ks, seed)
    x, h = make_inputs(Cx, Ch, B, H, W, seed)
    ref64 = torch_forward(state, x, h, torch.float64).numpy()
    return R.weights_of(state), x.numpy(), h.numpy(), ref64


def max_abs(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


@pytest.mark.parametrize("k", range(len(CASES)), ids=[str(c) for c in CASES])
def test_restatement_against_float64(k):
    worst = []
    for seed in MEASURED_SEEDS + (FIFTH_SEED,):
        state, x, h, ref64 = case(k, seed)
        worst.append(max_abs(R.forward(x, h, state), ref64))
    print(f"case {CASES[k]}: max |restatement - float64| per seed {['%.3g' % w for w in worst]} (measured maximum {MEASURED_MAX_ABS:.3g}, bound {BOUND:.3g})")
    assert max(worst[:-1]) <= MEASURED_MAX_ABS * 1.0001, "the recorded maximum is out of date"
    assert max(worst) <= BOUND


@pytest.mark.parametrize("name", sorted(R.MUTANTS))
def test_mutants_fail_the_float64_bound(name):
    worst = []
    for k in range(len(CASES)):
        state, x, h, ref64 = case(k, MEASURED_SEEDS[0])
        worst.append(max_abs(R.forward(x, h, state, variant=R.MUTANTS[name]), ref64))
    print(f"mutant {name}: {['%.3g' % w for w in worst]} (bound {BOUND:.3g})")
    assert min(worst) > BOUND


# ---- known answers -------------------------------------------------------------------------------------------------------------


def zero_state(Cx, Ch, ks):
    state = {}
    for g in R.GATES:
        state[f"conv_{g}.weight"] = np.zeros((Ch, Cx + Ch, 1, ks) if g.endswith("horizontal") else (Ch, Cx + Ch, ks, 1), np.float32)
        state[f"conv_{g}.bias"] = np.zeros(Ch, np.float32)
    return state


def test_saturated_update_gate():
    """All-zero weights: b_z = +40 makes z exactly 1, so h' = tanh_c(b_q) everywhere (of the vertical pass, the last one);
    b_z = -40 makes z = exp_c(-40) / (1 + exp_c(-40)): 1 - z rounds to 1 and z * q is below half an ulp of h, so h' = h bit for bit."""
    Cx, Ch, ks, B, H, W = 2, 3, 5, 2, 4, 5
    x, h = (t.numpy() for t in make_inputs(Cx, Ch, B, H, W, 7))
    bq = np.float32([0.3, -1.7, 0.01])
    state = zero_state(Cx, Ch, ks)
    for d in ("horizontal", "vertical"):
        state[f"conv_z_{d}.bias"][:] = 40.0
        state[f"conv_q_{d}.bias"][:] = bq
    want = np.broadcast_to(R.tanh_c(bq)[None, :, None, None], h.shape)
    assert R.same(R.forward(x, h, state), want)
    for d in ("horizontal", "vertical"):
        state[f"conv_z_{d}.bias"][:] = -40.0
    assert R.same(R.forward(x, h, state), h)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (3, 3)])
@pytest.mark.parametrize("vertical", [0, 1])
@pytest.mark.parametrize("t", range(5))
def test_single_tap_shows_direction_and_zero_padding(H, W, vertical, t):
    """One non-zero weight, q's tap t on input channel 0 (of x) in one pass, z saturated at 1 in that pass and at 0 in the other (which
    then is the identity): h' = tanh_c(x shifted by t - 2 along the pass direction), exactly +0 where the tap is outside the image."""
    ks, pad = 5, 2
    rng = np.random.default_rng(10 * H + W)
    x = rng.standard_normal((1, 1, H, W)).astype(np.float32)
    h = rng.standard_normal((1, 1, H, W)).astype(np.float32)
    state = zero_state(1, 1, ks)
    on, off = ("vertical", "horizontal") if vertical else ("horizontal", "vertical")
    state[f"conv_z_{on}.bias"][:] = 40.0
    state[f"conv_z_{off}.bias"][:] = -40.0
    state[f"conv_q_{on}.weight"].reshape(2, ks)[0, t] = 1.0
    shifted = np.zeros_like(x)
    for y in range(H):
        for xx in range(W):
            sy, sx = (y + t - pad, xx) if vertical else (y, xx + t - pad)
            if 0 <= sy < H and 0 <= sx < W:
                shifted[0, 0, y, xx] = x[0, 0, sy, sx]
    want = R.tanh_c(shifted)
    got = R.forward(x, h, state)
    assert R.same(got, want)  # the other pass is the identity: z * q = z * tanh_c(0) = 0 there
    assert not np.signbit(got[shifted == 0]).any()


def test_three_parts_equal_their_concatenation():
    state, x, h, _ = case(1, MEASURED_SEEDS[0])
    parts = (x[:, :100], x[:, 100:130], x[:, 130:])
    assert R.same(R.forward(parts, h, state), R.forward(x, h, state))


# ---- sigmoid_c and tanh_c against float64 --------------------------------------------------------------------------------------


def ulp_error(got, want):
    _, exponent = np.frexp(want)  # want = f * 2^exponent, f in [0.5, 1): its float32 ulp is 2^(exponent - 24)
    return np.abs(got.astype(np.float64) - want) / np.ldexp(1.0, exponent - 24)


def every_float32(lo, hi):
    return np.arange(np.float32(lo).view(np.int32), np.float32(hi).view(np.int32), dtype=np.int64).astype(np.int32).view(np.float32)


def test_tanh_c_against_float64():
    """Every float32 in [1/16, 1) (two binades on each side of the branch point 0.25) and 2 M log-spaced arguments from 1e-38 to 100,
    both signs."""
    assert R.tanh_small() == np.float32(0.25)
    v = np.concatenate([every_float32(0.0625, 1.0), np.exp(np.linspace(np.log(1e-38), np.log(100.0), 2_000_000)).astype(np.float32)])
    v = np.concatenate([v, -v])
    got = R.tanh_c(v)
    err = ulp_error(got, np.tanh(v.astype(np.float64)))
    worst = int(err.argmax())
    print(f"tanh_c over {v.size} arguments: max error {err.max():.3f} ulp at v = {float(v[worst])!r} (measured {TANH_C_ULP}, bound {TANH_C_ULP + 1})")
    assert err.max() <= TANH_C_ULP + 1
    assert np.array_equal(np.signbit(got), np.signbit(v)) and (np.abs(got) <= 1).all()


def test_sigmoid_c_against_float64():
    """Every float32 in [1/4, 4) and 2 M log-spaced arguments from 1e-38 to 87, both signs (sigmoid_c has no branch point of its own but
    the sign; exp_c's are the reduction boundaries, which the dense range crosses).  Below -87 exp_c cuts off and sigmoid_c is exactly +0
    where the float64 value is below 2^-125: that range is asserted as such, not in ulp."""
    v = np.concatenate([every_float32(0.25, 4.0), np.exp(np.linspace(np.log(1e-38), np.log(87.0), 2_000_000)).astype(np.float32)])
    v = np.concatenate([v, -v])
    got = R.sigmoid_c(v)
    err = ulp_error(got, 1.0 / (1.0 + np.exp(-v.astype(np.float64))))
    worst = int(err.argmax())
    print(f"sigmoid_c over {v.size} arguments: max error {err.max():.3f} ulp at v = {float(v[worst])!r} (measured {SIGMOID_C_ULP}, bound {SIGMOID_C_ULP + 1})")
    assert err.max() <= SIGMOID_C_ULP + 1
    below = -np.exp(np.linspace(np.log(87.001), np.log(1e30), 10_000)).astype(np.float32)
    out = R.sigmoid_c(below)
    assert (out == 0).all() and not np.signbit(out).any()


def test_saturation_nan_zero_and_subnormal_arguments():
    nan, tiny = np.float32("nan"), np.float32(1e-41)
    s = R.sigmoid_c(np.float32([200, -200, np.inf, -np.inf, nan, 0.0, -0.0, tiny, -tiny]))
    assert s[0] == 1 and s[1] == 0 and not np.signbit(s[1]) and s[2] == 1 and s[3] == 0 and np.isnan(s[4])
    assert (s[5:] == np.float32(0.5)).all()
    t = R.tanh_c(np.float32([200, -200, np.inf, -np.inf, nan, 0.0, -0.0, tiny, -tiny]))
    assert t[0] == 1 and t[1] == -1 and t[2] == 1 and t[3] == -1 and np.isnan(t[4])
    assert t[5] == 0 and not np.signbit(t[5]) and t[6] == 0 and np.signbit(t[6])
    assert t[7] == tiny and t[8] == -tiny  # tanh(v) = v to float32 for a subnormal v


# ---- the packed layout ---------------------------------------------------------------------------------------------------------


def test_packed_layout_is_the_headers():
    """SepConvGru packs [M][K] as [tile][k-step][64], lane = 32 (k % 2) + row % 32, -0 beyond K and +0 beyond M (include/ftk.h)."""
    import feature_tracker_amd as F
    from feature_tracker_amd import _native as N
    Cx, Ch, ks = 3, 40, 5
    state = make_state(Cx, Ch, ks, 3)
    gru = F.SepConvGru.from_state_dict(state)
    K, k_steps = (Cx + Ch) * ks, N.sep_conv_gru_k_steps(Cx + Ch, ks)
    assert k_steps == 3 * 40 and 2 * k_steps >= K
    for d in ("horizontal", "vertical"):
        zr = np.concatenate([state[f"conv_z_{d}.weight"].numpy().reshape(Ch, K), state[f"conv_r_{d}.weight"].numpy().reshape(Ch, K)])
        for key, matrix in (("zr_" + d, zr), ("q_" + d, state[f"conv_q_{d}.weight"].numpy().reshape(Ch, K))):
            packed = gru._packed[key].numpy()
            M = matrix.shape[0]
            assert packed.size == N.sep_conv_gru_packed_elements(M, Cx + Ch, ks)
            packed = packed.reshape(-1, k_steps, 2, 32)
            for row, k in itertools.product((0, 1, 31, 32, M - 1), (0, 1, 2, K - 1)):
                assert packed[row // 32, k // 2, k % 2, row % 32] == matrix[row, k]
            beyond_k = packed[:, K // 2:, :, :].reshape(packed.shape[0], -1, 32)[:, (K % 2):, :]
            assert (beyond_k == 0).all() and np.signbit(beyond_k).all()
            beyond_m = packed[M // 32, :K // 2, :, M % 32:]
            assert (beyond_m == 0).all() and not np.signbit(beyond_m).any()
        assert np.array_equal(gru._packed["zr_bias_" + d].numpy(), np.concatenate([state[f"conv_z_{d}.bias"].numpy(), state[f"conv_r_{d}.bias"].numpy()]))
    if os.path.exists(N.LIB_PATH):
        import ctypes as C
        e = C.c_int64()
        assert N.lib().ftk_sep_conv_gru_packed_elements(2 * Ch, Cx + Ch, ks, C.byref(e)) == 0 and e.value == N.sep_conv_gru_packed_elements(2 * Ch, Cx + Ch, ks)


# ---- loud failures, before any device is touched -------------------------------------------------------------------------------


def test_from_state_dict_refuses_by_key():
    import feature_tracker_amd as F
    state = make_state(3, 16, 5, 1)
    gru = F.SepConvGru.from_state_dict(state)
    assert (gru.x_channels, gru.h_channels, gru.kernel_size) == (3, 16, 5) and set(gru.weights) == set(state)
    whole = {"update_block.gru." + k: v for k, v in state.items()}
    assert F.SepConvGru.from_state_dict(whole, prefix="update_block.gru.").h_channels == 16
    with pytest.raises(ValueError, match="conv_z_horizontal.weight"):
        F.SepConvGru.from_state_dict(whole)  # no prefix: the key is missing
    for key, bad, match in (("conv_r_vertical.weight", state["conv_r_vertical.weight"].double(), "conv_r_vertical.weight must be a float32"),
                            ("conv_q_horizontal.bias", torch.zeros(17), r"conv_q_horizontal.bias must be .*\[16\]"),
                            ("conv_z_vertical.weight", state["conv_z_horizontal.weight"], r"conv_z_vertical.weight must be .*\[16, 19, 5, 1\]"),
                            ("conv_q_vertical.bias", None, "conv_q_vertical.bias is missing")):
        broken = dict(state)
        if bad is None:
            del broken[key]
        else:
            broken[key] = bad
        with pytest.raises(ValueError, match=match):
            F.SepConvGru.from_state_dict(broken)
    with pytest.raises(ValueError, match="kernel_size 7 is not supported"):
        F.SepConvGru.from_state_dict(make_state(3, 16, 7, 1))
    with pytest.raises(ValueError, match="kernel_size 7 is not supported"):
        F.SepConvGru(3, 16, 7)
    with pytest.raises(ValueError, match="h_channels"):
        F.SepConvGru(3, 1025)
    with pytest.raises(ValueError, match="x_channels"):
        F.SepConvGru(0, 16)
    with pytest.raises(ValueError, match="above 4096"):
        F.SepConvGru(4000, 512)
    F.SepConvGru(512, 512)  # C_in = 1024 and h_channels = 512 are inside the limits


def test_wrapper_refuses_bad_arguments_without_a_device():
    import feature_tracker_amd as F
    gru = F.SepConvGru.from_state_dict(make_state(35, 16, 5, 1))
    x, h = torch.zeros(2, 35, 3, 5), torch.zeros(2, 16, 3, 5)
    parts = (x[:, :3], x[:, 3:33], x[:, 33:])
    bad = [
        ("x must be", (x.double(), h)), ("h must be", (x, h.half())), ("h must be", (x, h[0])), ("x must be", (x.numpy(), h)),   # dtype, rank, type
        (r"x\[1\] must be", ((parts[0], parts[1].double(), parts[2]), h)),
        ("h has 17 channels", (x, torch.zeros(2, 17, 3, 5))),
        ("agree", (x, torch.zeros(2, 16, 4, 5))), ("agree", (torch.zeros(3, 35, 3, 5), h)), ("agree", ((parts[0], parts[1], torch.zeros(2, 2, 3, 6)), h)),
        ("channels of x sum to 34", (x[:, :34], h)), ("channels of x sum to 33", (parts[:2], h)),
        ("sequence of 1 .. 3", ((parts[0], parts[1], x[:, 33:34], x[:, 34:]), h)), ("sequence of 1 .. 3", ((), h)), ("must be a tensor or a sequence", (None, h)),
    ]
    for match, args in bad:
        with pytest.raises(ValueError, match=match):
            gru(*args)
    with pytest.raises(RuntimeError, match="inference only"):
        gru(x.clone().requires_grad_(True), h)
    with pytest.raises(RuntimeError, match="inference only"):
        gru((parts[0], parts[1].clone().requires_grad_(True), parts[2]), h)
    with torch.no_grad(), pytest.raises(ValueError, match="no CPU fallback"):
        gru(x.clone().requires_grad_(True), h)
    for args in ((x, h), (parts, h)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            gru(*args)
    with pytest.raises(ValueError, match="no weights yet"):
        F.SepConvGru(35, 16)(x, h)


def test_device_entry_refuses_bad_arguments_without_a_device():
    import feature_tracker_amd as F
    from feature_tracker_amd import device as D
    ctx = types.SimpleNamespace(handle=None)
    gru = F.SepConvGru.from_state_dict(make_state(3, 16, 5, 1))
    x, h = torch.zeros(1, 3, 3, 5), torch.zeros(1, 16, 3, 5)
    bufs = [torch.zeros(1, 16, 3, 5) for _ in range(4)]
    with pytest.raises(ValueError, match="^h must be a CUDA tensor"):
        D.sep_conv_gru_device(ctx, [x], h, gru._packed, 5, *bufs)
    with pytest.raises(ValueError, match="^h must be .*wrong dtype"):
        D.sep_conv_gru_device(ctx, [x], h.double(), gru._packed, 5, *bufs)
    with pytest.raises(ValueError, match="kernel_size 7"):
        D.sep_conv_gru_device(ctx, [x], h, gru._packed, 7, *bufs)
    with pytest.raises(ValueError, match="1 .. 3 tensors"):
        D.sep_conv_gru_device(ctx, [x] * 4, h, gru._packed, 5, *bufs)


# the walk of tests/args_walk.py (duck-typed tensors, a recording stand-in for the native library) over this entry
WALK_TENSORS = 2 + 1 + 4 + 8  # two x parts, h, z / rh / mid / out, the packed eight


def _walk_call(w):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    from feature_tracker_amd._device_sep_conv_gru import PACKED_KEYS
    B, Cx, Ch, H, W, ks = 2, 5, 40, 3, 7, 5
    parts = [w.t("x[0]", "float32", B, 3, H, W), w.t("x[1]", "float32", B, 2, H, W)]
    h = w.t("h", "float32", B, Ch, H, W)
    bufs = [w.t(name, "float32", B, Ch, H, W) for name in ("z", "rh", "mid", "out")]
    packed = {}
    for key in PACKED_KEYS:
        rows = Ch if key.startswith("q") else 2 * Ch
        packed[key] = w.t(f"packed['{key}']", "float32", rows if "bias" in key else N.sep_conv_gru_packed_elements(rows, Cx + Ch, ks))
    return D.sep_conv_gru_device(w.ctx, parts, h, packed, ks, *bufs)


def test_device_entry_takes_no_pointer_of_an_unchecked_argument(monkeypatch):
    w = A.walk_call(monkeypatch, _walk_call, ["ftk_sep_conv_gru_gates_device", "ftk_sep_conv_gru_blend_device"] * 2)
    assert len(w.made) == WALK_TENSORS


@pytest.mark.parametrize("which", range(WALK_TENSORS))
@pytest.mark.parametrize("kind", ["dtype", "shape", "device"])
def test_device_entry_stops_before_the_library(monkeypatch, which, kind):
    """Each tensor of the call in turn made float64, one element longer in its last dimension, or moved to another device."""
    w = A.Walk(monkeypatch, spoil=(which, kind, A.one_column_more if kind == "shape" else None))
    with pytest.raises(ValueError) as e:
        _walk_call(w)
    name = w.spoiled.name
    if not (kind == "shape" and name == "h"):  # a longer h is a legal h: the first x part is then the one refused
        assert name.replace("'", "") in str(e.value).replace("'", ""), (name, str(e.value))
    assert w.lib.calls == [] and w.unchecked_reads == []


# ---- the launch plan -----------------------------------------------------------------------------------------------------------

LDS_PER_WORKGROUP = 160 * 1024  # MI355X: 160 KiB of LDS per CU, all of it available to one workgroup
PLAN_FIELDS = ("h_channels", "in_channels", "kernel_size", "vertical", "gates", "B", "H", "W")


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
    cases = []
    for (h, x), ks, vertical, gates, (B, H, W) in itertools.product(
            ((1, 1), (16, 3), (33, 1), (40, 131), (48, 16), (64, 160), (96, 2), (128, 256), (256, 131), (512, 512), (1024, 3072)), (3, 5), (0, 1), (0, 1),
            ((1, 1, 1), (2, 6, 7), (1, 1, 7), (1, 7, 1), (1, 3, 3), (1, 2, 131), (1, 55, 128), (3, 33, 129), (1, 1, 100000), (1, 100000, 1))):
        cases.append(dict(h_channels=h, in_channels=h + x, kernel_size=ks, vertical=vertical, gates=gates, B=B, H=H, W=W))
    seen_wm = set()
    for c, p in zip(cases, plan(cases)):
        what = f"{c} -> {p}"
        assert p["refused"] == "none", what
        M = (2 if c["gates"] else 1) * c["h_channels"]
        pad = c["kernel_size"] // 2
        seen_wm.add(p["wm"])
        assert p["out_channels"] == M and p["m_tiles"] == cdiv(M, 32) and p["wm"] * p["wn"] == 4 and p["wm"] in (1, 2, 4), what
        # every output channel and pixel belongs to exactly one (workgroup, wave, MFMA tile): the row tiles of the workgroups along y
        # partition the channel tiles, their pixel tiles partition the image, tile after tile without overlap
        assert p["m_groups"] == cdiv(p["m_tiles"], p["wm"]) and (p["m_groups"] - 1) * p["wm"] < p["m_tiles"], what
        assert (p["tile_w"], p["tile_h"]) == ((32, p["wn"]) if c["vertical"] else (32 * p["wn"], 1)), what
        assert p["tiles_x"] * p["tile_w"] >= c["W"] > (p["tiles_x"] - 1) * p["tile_w"], what
        assert p["tiles_y"] * p["tile_h"] >= c["H"] > (p["tiles_y"] - 1) * p["tile_h"], what
        assert p["grid"] == (p["tiles_x"] * p["tiles_y"] * c["B"], p["m_groups"]) and p["block"] == (256, 1), what
        assert p["grid"][0] < 2 ** 31 and p["grid"][1] <= 65535, what
        # the chunks cover every k in order, in whole k-steps
        assert p["chunk"] == 16 and p["chunks"] == cdiv(c["in_channels"], 16) and p["steps_per_chunk"] * 2 == 16 * c["kernel_size"], what
        assert p["k_steps"] == p["chunks"] * p["steps_per_chunk"] and 2 * p["k_steps"] >= c["in_channels"] * c["kernel_size"], what
        assert p["packed"] == p["m_tiles"] * p["k_steps"] * 64, what
        # LDS: the strip and its halo, inside the kernel's static array, inside the device's limit
        strip = (p["wn"] + 2 * pad) * 32 if c["vertical"] else 32 * p["wn"] + 2 * pad
        assert p["pitch"] == strip and p["lds"] == 16 * strip * 4 <= p["lds_static"] <= LDS_PER_WORKGROUP, what
        assert p["mfma"] == "32x32x2_f32", what
    assert seen_wm == {1, 2, 4}


def test_plan_refuses_limits_by_name():
    base = dict(h_channels=16, in_channels=19, kernel_size=5, vertical=0, gates=1, B=1, H=4, W=4)
    cases = [dict(base, kernel_size=7), dict(base, kernel_size=1), dict(base, h_channels=0), dict(base, h_channels=1025, in_channels=1030),
             dict(base, in_channels=16), dict(base, in_channels=4097), dict(base, B=0), dict(base, W=0), dict(base, H=-1),
             dict(base, B=2 ** 31 - 1, H=2 ** 31 - 1), dict(base, h_channels=1024, in_channels=4096), dict(base, h_channels=512, in_channels=1024)]
    got = [p["refused"] for p in plan(cases)]
    assert got == ["kernel_size", "kernel_size", "h_channels", "h_channels", "in_channels", "in_channels", "sizes", "sizes", "sizes", "grid", "none", "none"]


def test_plan_counts_tiles_of_the_widest_row_exactly():
    """W + tile_w - 1 passes 2^31 for a W near INT32_MAX: the tile counts are computed in 64 bits, for every wave split, and the grid is
    refused only when the workgroup count itself passes 2^31 - 1."""
    W = 2 ** 31 - 1
    cases = [dict(h_channels=h, in_channels=h + 16, kernel_size=ks, vertical=vertical, gates=0, B=1, H=1, W=W)
             for h in (16, 48, 100) for vertical in (0, 1) for ks in (3, 5)]
    plans = plan(cases)
    assert sorted({p.get("wn") for p in plans}) == [1, 2, 4]
    for c, p in zip(cases, plans):
        what = f"{c} -> {p}"
        assert p["refused"] == "none", what
        assert p["wn"] == {16: 4, 48: 2, 100: 1}[c["h_channels"]], what
        assert p["tile_w"] == (32 if c["vertical"] else 32 * p["wn"]), what
        assert p["tiles_x"] == cdiv(W, p["tile_w"]) and p["tiles_y"] == 1, what
        assert p["grid"] == (cdiv(W, p["tile_w"]), p["m_groups"]), what
    refused = plan([dict(c, B=2 ** 31 - 1, H=1, W=129) for c in cases])
    assert [p["refused"] for p in refused] == ["grid"] * len(cases)
