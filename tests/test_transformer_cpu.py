"""The scalar restatement of LightGlue's transformer layer (tests/transformer_ref.c) pinned without a device: known
answers by hand, erf_c's error bound, upstream's formulas in torch float64, and the mutants.

Measured here against float64 at the GPU tests' shapes (transformer_ref.LAYER_SHAPES, with and without counts): the worst absolute
deviation of an output element is MEASURED_DEVIATION; the bound is 4 x that (DESIGN.md 5.23's margin).  erf_c's worst error against
float64 erf over 2^20 + 1 points of [-6, 6] and every float32 of [2^-40, 2^-10] step 4099 is MEASURED_ERF_ULP; the bound is the next
whole ulp above it.

Measured the same way at the shapes of the non-vector path (transformer_ref.LAYER_NARROW, with and without counts): MEASURED_DEVIATION_NARROW.
With both blocks' LayerNorm weight times transformer_ref.GELU_WEIGHT_SCALE (the case that takes every branch of erf_c) the weight
multiplies the error and the outputs are about 26 in magnitude instead of about 3: MEASURED_DEVIATION_SCALED, at LAYER_SHAPES[2].  Each
has its own bound of 4 x its constant; every one of them measures the restatement against float64, never the device."""
import functools
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import transformer_ref as R  # noqa: E402

MEASURED_ERF_ULP = 2.3746
ERF_ULP_BOUND = 3.0
MEASURED_DEVIATION = 4.063e-6  # at (130, 65, 256, 4) with counts
DEVIATION_BOUND = 4 * MEASURED_DEVIATION
MEASURED_DEVIATION_NARROW = 2.673e-6  # at (35, 33, 130, 5) with counts
DEVIATION_BOUND_NARROW = 4 * MEASURED_DEVIATION_NARROW
MEASURED_DEVIATION_SCALED = 5.208e-5  # at (65, 130, 64, 4) with counts, LayerNorm weights x 6
DEVIATION_BOUND_SCALED = 4 * MEASURED_DEVIATION_SCALED


# ---- known answers -----------------------------------------------------------------------------------------------------------------------

def test_one_key_gives_its_value_row():
    q, k, v = R.qkv(5, 1, 2, 4, 1)
    out = R.attention(q, k, v)
    assert R.same(out, np.broadcast_to(v, out.shape))  # p = exp_c(0) / 1 = 1, and fmaf(1, v, +0) = v
    q, k, v = R.qkv(5, 9, 2, 4, 2)
    assert R.same(R.attention(q, k, v, count=1), np.broadcast_to(v[:1], (5, 2, 4)))


def test_identical_keys_give_the_mean_of_the_values_to_the_stated_roundings():
    for n in (2, 3, 7, 64, 65, 130):
        q, k, v = (np.array(x, copy=True) for x in R.qkv(3, n, 1, 4, 3))
        k[:] = k[0]
        p = np.float32(1.0) / np.float32(n)  # every s equals m: exp_c(0) = 1; l = n exactly (the tree adds small integers); p = 1 / n rounded once
        want = np.zeros((3, 1, 4), np.float32)
        for j in range(n):  # the fmaf chain over ascending keys
            want = (p.astype(np.float64) * v[j].astype(np.float64) + want.astype(np.float64)).astype(np.float32)
        assert R.same(R.attention(q, k, v), want)


def test_a_zero_rotary_angle_is_the_identity():
    rng = np.random.default_rng(4)
    t = rng.standard_normal((7, 12)).astype(np.float32)
    enc = np.stack([np.ones((7, 4), np.float32), np.zeros((7, 4), np.float32)])
    assert R.same(R.rotary(t, 3, enc), t + np.float32(0.0))  # x * 1 + (-y) * 0 = x (-0 becomes +0, which `+ 0.0` states)


def test_no_valid_key_gives_positive_zero():
    q, k, v = R.qkv(4, 6, 2, 4, 5)
    for count in (0, -2):
        out = R.attention(q, k, v, count=count)
        assert (out == 0).all() and not np.signbit(out).any()


def test_the_float32_torch_rotary_equals_the_restatements_bit_for_bit():
    """upstream's apply_cached_rotary_emb: (t * cos) + (rotate_half(t) * sin), in torch float32 on the CPU"""
    m, n, d, h, seed = R.LAYER_SHAPES[2]
    a, _, kp0, _, size = R.inputs(m, n, d, h, seed)
    enc = R.encoding(kp0, size, R.state_dict(d, h, 1, seed + 1000)["posenc.Wr.weight"])
    t = torch.from_numpy(a.copy()).view(m, h, d // h)
    freqs = torch.from_numpy(enc).unsqueeze(-2)  # [2, m, 1, dh]
    pairs = t.unflatten(-1, (-1, 2))
    x1, x2 = pairs.unbind(dim=-1)
    rotated = torch.stack((-x2, x1), dim=-1).flatten(start_dim=-2)
    want = (t * freqs[0]) + (rotated * freqs[1])
    assert R.same(R.rotary(a, h, enc), want.reshape(m, d).numpy())
    assert not R.same(R.rotary(a, h, enc, R.MUTANTS["rotary_pairs_as_halves"]), want.reshape(m, d).numpy())


# ---- erf_c -------------------------------------------------------------------------------------------------------------------------------

def _ulp_error(got, x):
    want = np.array([math.erf(float(v)) for v in x])
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want) / ulp


def test_erf_c_within_its_stated_bound_and_odd():
    grid = np.linspace(-6.0, 6.0, (1 << 20) + 1).astype(np.float32)
    tiny = np.arange(np.float32(2.0 ** -40).view(np.uint32), np.float32(2.0 ** -10).view(np.uint32), 4099, dtype=np.uint32).view(np.float32)
    x = np.concatenate([grid, tiny, -tiny, np.float32([1.0, 4.0, -1.0, -4.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(4), np.float32(0))])])
    got = R.erf_c(x)
    worst = _ulp_error(got, x).max()
    print(f"erf_c: worst error {worst:.4f} ulp")
    assert worst <= ERF_ULP_BOUND
    assert R.same(R.erf_c(-x), -got)
    zeros = R.erf_c(np.float32([0.0, -0.0]))
    assert zeros[0] == 0 and zeros[1] == 0 and not np.signbit(zeros[0]) and np.signbit(zeros[1])
    assert np.isnan(R.erf_c(np.float32([np.nan])))[0] and R.same(R.erf_c(np.float32([np.inf, -np.inf, 7.0])), np.float32([1, -1, 1]))


# ---- upstream's formulas in float64 ------------------------------------------------------------------------------------------------------

def _t(x):
    return torch.from_numpy(np.asarray(x)).double()


def _attention64(q, k, v, n):
    """upstream's Attention on [h, rows, dh] with the keys behind n masked out; n = 0: zeros"""
    if n == 0:
        return torch.zeros_like(q)
    s = torch.einsum("hid,hjd->hij", q, k[:, :n]) * q.shape[-1] ** -0.5
    return torch.einsum("hij,hjd->hid", torch.softmax(s, -1), v[:, :n])


def _ffn64(x, msg, sd, p):
    F = torch.nn.functional
    hid = F.linear(torch.cat([x, msg], -1), _t(sd[p + "ffn.0.weight"]), _t(sd[p + "ffn.0.bias"]))
    hid = F.gelu(F.layer_norm(hid, (hid.shape[-1],), _t(sd[p + "ffn.1.weight"]), _t(sd[p + "ffn.1.bias"]), 1e-5))
    return x + F.linear(hid, _t(sd[p + "ffn.3.weight"]), _t(sd[p + "ffn.3.bias"]))


def _rotary64(t, enc):
    x1, x2 = t.unflatten(-1, (-1, 2)).unbind(dim=-1)
    return t * enc[0] + torch.stack((-x2, x1), dim=-1).flatten(start_dim=-2) * enc[1]


def _self64(x, enc, n, sd, p, h):
    F = torch.nn.functional
    rows, d = x.shape
    qkv = F.linear(x, _t(sd[p + "Wqkv.weight"]), _t(sd[p + "Wqkv.bias"])).unflatten(-1, (h, -1, 3)).transpose(0, 1)  # [h, rows, dh, 3]
    q, k, v = qkv[..., 0], qkv[..., 1], qkv[..., 2]
    ctx = _attention64(_rotary64(q, enc), _rotary64(k, enc), v, n).transpose(0, 1).reshape(rows, d)
    return _ffn64(x, F.linear(ctx, _t(sd[p + "out_proj.weight"]), _t(sd[p + "out_proj.bias"])), sd, p)


def layer64(desc0, desc1, h, enc0, enc1, sd, prefix="transformers.0.", count0=None, count1=None):
    """upstream's TransformerLayer (SelfBlock on each set, CrossBlock) in torch float64 on the CPU"""
    F = torch.nn.functional
    x0, x1, e0, e1 = _t(desc0), _t(desc1), _t(enc0).unsqueeze(1), _t(enc1).unsqueeze(1)  # enc: [2, 1, rows, dh]
    (m, d), n = x0.shape, x1.shape[0]
    n0 = m if count0 is None else min(max(count0, 0), m)
    n1 = n if count1 is None else min(max(count1, 0), n)
    x0, x1 = _self64(x0, e0, n0, sd, prefix + "self_attn.", h), _self64(x1, e1, n1, sd, prefix + "self_attn.", h)
    p = prefix + "cross_attn."
    heads = lambda t: t.unflatten(-1, (h, -1)).transpose(0, 1)  # noqa: E731
    qk0, qk1 = (heads(F.linear(x, _t(sd[p + "to_qk.weight"]), _t(sd[p + "to_qk.bias"]))) for x in (x0, x1))
    v0, v1 = (heads(F.linear(x, _t(sd[p + "to_v.weight"]), _t(sd[p + "to_v.bias"]))) for x in (x0, x1))
    m0 = _attention64(qk0, qk1, v1, n1).transpose(0, 1).reshape(m, d)  # q k^T dh^-0.5 = (q dh^-0.25)(k dh^-0.25)^T
    m1 = _attention64(qk1, qk0, v0, n0).transpose(0, 1).reshape(n, d)
    m0, m1 = (F.linear(t, _t(sd[p + "to_out.weight"]), _t(sd[p + "to_out.bias"])) for t in (m0, m1))
    return _ffn64(x0, m0, sd, p).numpy(), _ffn64(x1, m1, sd, p).numpy()


def _counts(shape, counted):
    m, n = shape[:2]
    return ((2 * m + 2) // 3, (3 * n + 3) // 4) if counted else (None, None)


@functools.lru_cache(maxsize=None)
def _reference(shape, counted):
    a, b, e0, e1, sd = R.layer_case(shape)
    c0, c1 = _counts(shape, counted)
    return layer64(a, b, shape[3], e0, e1, sd, count0=c0, count1=c1)


def _deviation(shape, counted, variant=R.CONTRACT):
    a, b, e0, e1, sd = R.layer_case(shape)
    c0, c1 = _counts(shape, counted)
    got = R.layer(a, b, shape[3], e0, e1, sd, count0=c0, count1=c1, variant=variant)
    want = _reference(shape, counted)
    return max(np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max())  # (rows behind a count are queries like any other, in both)


@pytest.mark.parametrize("counted", [False, True], ids=["all_rows", "with_counts"])
@pytest.mark.parametrize("shape", R.LAYER_SHAPES, ids=["x".join(str(v) for v in s[:4]) for s in R.LAYER_SHAPES])
def test_the_restatement_against_upstreams_formulas_in_float64(shape, counted):
    worst = _deviation(shape, counted)
    print(f"{shape[:4]} counted={counted}: worst absolute deviation {worst:.3e}")
    assert worst <= DEVIATION_BOUND


@pytest.mark.parametrize("counted", [False, True], ids=["all_rows", "with_counts"])
@pytest.mark.parametrize("shape", R.LAYER_NARROW, ids=["x".join(str(v) for v in s[:4]) for s in R.LAYER_NARROW])
def test_the_restatement_against_float64_at_the_shapes_of_the_non_vector_path(shape, counted):
    assert shape[2] % 4 != 0
    worst = _deviation(shape, counted)
    print(f"{shape[:4]} counted={counted}: worst absolute deviation {worst:.3e}")
    assert worst <= DEVIATION_BOUND_NARROW


@pytest.mark.parametrize("counted", [False, True], ids=["all_rows", "with_counts"])
def test_the_scaled_layernorm_weight_takes_every_branch_of_erf_c_and_stays_at_float64(counted):
    """The inputs of the GPU test of the same case: every branch of erf_c holds at least 1 % of the self block's pre-GELU values of
    either set (a condition on the inputs; about 19 % / 47 % / 34 % here, against 84 % / 16 % / 0 with the weights as they are), the
    restatement's outputs are finite, and they stay at upstream's formulas in float64."""
    shape = R.LAYER_SHAPES[2]
    h = shape[3]
    a, b, e0, e1, sd = R.scaled_gelu_case(shape)
    c0, c1 = _counts(shape, counted)
    for x, enc, count in ((a, e0, c0), (b, e1, c1)):
        shares = R.erf_branch_shares(R.self_block_pre_gelu(x, h, enc, sd, count))
        print(f"counted={counted}: shares of a < 1, 1 <= a < 4, a >= 4: " + " / ".join(f"{100 * s:.1f} %" for s in shares))
        assert min(shares) >= 0.01
    plain = R.layer_case(shape)
    assert R.erf_branch_shares(R.self_block_pre_gelu(plain[0], h, plain[2], plain[4]))[2] == 0  # what the other layer tests leave out
    got = R.layer(a, b, h, e0, e1, sd, count0=c0, count1=c1)
    want = layer64(a, b, h, e0, e1, sd, count0=c0, count1=c1)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    worst = max(np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max())
    print(f"counted={counted}: worst absolute deviation {worst:.3e}")
    assert worst <= DEVIATION_BOUND_SCALED


def test_the_hostile_layer_case_spoils_only_its_own_rows_and_overflows_a_variance():
    """The inputs of the GPU test of the same case, on the restatement alone: the rows that hold a NaN or an inf, and the row of 3e38,
    whose Linears overflow, come out all NaN; every other row is finite, the row of zeros (variance 0) and the subnormal row among them; and the
    row of 1e30 reaches LayerNorm finite, its sum of squares overflows, rstd is 0 and the row leaves the layer finite."""
    shape = R.LAYER_SHAPES[2]
    h = shape[3]
    a, b, e0, e1, sd = R.hostile_layer_case(shape)
    c0, c1 = R.HOSTILE_COUNTS
    out0, out1 = R.layer(a, b, h, e0, e1, sd, count0=c0, count1=c1)
    assert np.flatnonzero(~np.isfinite(out0).all(1)).tolist() == [3] and np.flatnonzero(~np.isfinite(out1).all(1)).tolist() == [8, 9]
    assert np.isnan(out0[3]).all() and np.isnan(out1[8]).all() and np.isnan(out1[9]).all()
    assert np.isfinite(b[8]).all() and not np.isfinite(b[9]).all() and not np.isfinite(a[3]).all()  # row 8 entered finite
    hid = R.self_block_hidden(b, h, e1, sd, c1)
    assert np.isfinite(hid[7]).all() and not np.isfinite(hid[8]).any()
    with np.errstate(over="ignore"):
        dev = hid[7] - np.float32(hid[7].astype(np.float64).mean())
        assert np.isfinite(dev).all() and np.isinf((dev * dev).sum(dtype=np.float32))
    gamma_beta = [sd[f"transformers.0.self_attn.ffn.1.{part}"] for part in ("weight", "bias")]
    normed = R.layernorm_gelu(hid[7:8], *gamma_beta)
    assert R.same(normed, R.layernorm_gelu(np.zeros((1, hid.shape[1]), np.float32), np.zeros_like(gamma_beta[0]), gamma_beta[1]))  # y = beta: rstd was 0


@pytest.mark.parametrize("case", R.LINEAR_HOSTILE, ids=lambda c: f"{c[0]}x{c[1]}to{c[2]}")
def test_the_hostile_linear_case_holds_nan_finite_values_and_a_negative_zero(case):
    x, w, bias = R.hostile_linear_case(*case)
    for a in (x, w, bias):
        assert np.isnan(a).any() and np.isinf(a).any() and ((a == 0) & np.signbit(a)).any() and ((a != 0) & (np.abs(a) < 1.1754944e-38)).any()
    assert not x[2].any() and not np.signbit(x[2]).any() and np.signbit(bias[1]) and np.signbit(bias[4])
    want = R.linear(x, w, bias)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).sum() > want.size // 2
    assert want[2, 1] == 0 and np.signbit(want[2, 1])      # -0 + (+0)(w < 0) ... stays -0
    assert want[2, 4] == 0 and not np.signbit(want[2, 4])  # -0 + (+0)(w > 0) is +0
    for k in range(1, case[1] + 1):  # the chain cut anywhere (a k-step padded with a product of -0 adds nothing to either)
        part = R.linear(x[2:3, :k], w[:, :k], bias)
        assert np.signbit(part[0, 1]) and not np.signbit(part[0, 4])


def test_the_linear_cases_cover_every_edge_named():
    assert len(R.LINEAR_CASES) < 40 and (33, 1024, 129) in R.LINEAR_CASES and (1, 1, 1) in R.LINEAR_CASES
    for axis, values in enumerate((R.LINEAR_ROWS, R.LINEAR_INS, R.LINEAR_OUTS)):
        assert {c[axis] for c in R.LINEAR_CASES} == set(values)
    assert R.LINEAR_HOSTILE == ((33, 5, 33), (33, 8, 33))


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_every_mutant_exceeds_the_bound(mutant):
    shape = R.LAYER_SHAPES[2]
    worst = _deviation(shape, True, R.MUTANTS[mutant])
    print(f"{mutant}: {worst:.3e}")
    assert worst > DEVIATION_BOUND
