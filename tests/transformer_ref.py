"""ctypes binding of tests/transformer_ref.c — the scalar CPU restatement of LightGlue's transformer layer — with the
shapes and seeded inputs the CPU and GPU tests share.

TEST INFRASTRUCTURE ONLY: compiled on first use (gcc -O3 -ffp-contract=off) into a temporary directory; nothing under
feature_tracker_amd/ may import it, and it imports nothing from there.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests.ref_build import compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "transformer_ref.c")

CONTRACT = 0
MUTANTS = {"rotary_pairs_as_halves": 1, "qkv_columns_as_3_h_dh": 2, "reverse_cross_softmax_along_the_wrong_axis": 3, "invalid_keys_inside_a_softmax": 4,
           "cat_order_msg_then_x": 5, "unbiased_layernorm_variance": 6}
# upstream's tensor names of one layer, in the order tests/transformer_ref.c reads them (weight, then bias, each)
LAYER_TENSORS = ("self_attn.Wqkv", "self_attn.out_proj", "self_attn.ffn.0", "self_attn.ffn.1", "self_attn.ffn.3", "cross_attn.to_qk", "cross_attn.to_v",
                 "cross_attn.to_out", "cross_attn.ffn.0", "cross_attn.ffn.1", "cross_attn.ffn.3")


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("transformer_ref", [_SRC])
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    for name in ("tr_exp_c", "tr_erf_c"):
        getattr(l, name).argtypes = [f32]
        getattr(l, name).restype = f32
    l.tr_linear.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, vp, vp]
    l.tr_linear.restype = None
    l.tr_rotary.argtypes = [vp, i32, i32, i32, vp, i32]
    l.tr_rotary.restype = None
    l.tr_attention.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, f32, f32, vp]
    l.tr_attention.restype = None
    l.tr_layernorm_gelu.argtypes = [vp, i32, i32, vp, vp, i32]
    l.tr_layernorm_gelu.restype = None
    l.tr_layer_weight_floats.argtypes = [i32]
    l.tr_layer_weight_floats.restype = C.c_int64
    l.tr_layer.argtypes = [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp]
    l.tr_layer.restype = i32
    return l


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _word(c):
    return None if c is None else np.array([c], np.int32)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def erf_c(x) -> np.ndarray:
    f = lib().tr_erf_c
    return np.array([f(float(v)) for v in np.asarray(x, np.float32).ravel()], np.float32)


def linear(x, weight, bias, xb=None, residual=None) -> np.ndarray:
    x, weight, bias = _f32(x), _f32(weight), _f32(bias)
    xb = None if xb is None else _f32(xb)
    residual = None if residual is None else _f32(residual)
    rows, ka = x.shape
    kb = 0 if xb is None else xb.shape[1]
    assert weight.shape == (bias.shape[0], ka + kb)
    out = np.empty((rows, weight.shape[0]), np.float32)
    lib().tr_linear(_p(x), _p(xb), rows, ka, kb, _p(weight), _p(bias), weight.shape[0], _p(residual), _p(out))
    return out


def rotary(t, heads, enc, variant=CONTRACT) -> np.ndarray:
    out, enc = np.array(t, np.float32, copy=True, order="C"), _f32(enc)
    rows, d = out.shape
    assert enc.shape == (2, rows, d // heads)
    lib().tr_rotary(_p(out), rows, d, heads, _p(enc), int(variant))
    return out


def default_post(dh: int) -> float:
    """The self block's (float)(1 / sqrt((double)dh))."""
    return float(np.float32(1.0 / np.sqrt(np.float64(dh))))


def cross_pre(dh: int) -> float:
    """The cross block's (float)pow((double)dh, -0.25)."""
    return float(np.float32(np.float64(dh) ** -0.25))


def attention(q, k, v, count=None, pre=1.0, post=None) -> np.ndarray:
    """q [M, h, dh], k and v [N, h, dh] -> [M, h, dh]."""
    q, k, v = _f32(q), _f32(k), _f32(v)
    m, h, dh = q.shape
    n = k.shape[0]
    assert k.shape == (n, h, dh) and v.shape == (n, h, dh)
    out = np.empty_like(q)
    word = _word(count)
    lib().tr_attention(_p(q), _p(k), _p(v), m, n, h * dh, h, _p(word), float(np.float32(pre)), default_post(dh) if post is None else float(np.float32(post)),
                       _p(out))
    return out


def layernorm_gelu(x, gamma, beta, variant=CONTRACT) -> np.ndarray:
    out = np.array(x, np.float32, copy=True, order="C")
    lib().tr_layernorm_gelu(_p(out), out.shape[0], out.shape[1], _p(_f32(gamma)), _p(_f32(beta)), int(variant))
    return out


def flat_weights(sd, prefix):
    """A layer's tensors of an upstream-style dict of numpy arrays as the one array tests/transformer_ref.c reads."""
    parts = [np.asarray(sd[f"{prefix}{name}.{part}"], np.float32).ravel() for name in LAYER_TENSORS for part in ("weight", "bias")]
    return np.ascontiguousarray(np.concatenate(parts))


def layer(desc0, desc1, heads, enc0, enc1, sd, prefix="transformers.0.", count0=None, count1=None, variant=CONTRACT):
    """(desc0', desc1') of one layer; ``sd``: upstream's names to numpy arrays."""
    desc0, desc1, enc0, enc1 = _f32(desc0), _f32(desc1), _f32(enc0), _f32(enc1)
    (m, d), n = desc0.shape, desc1.shape[0]
    w = flat_weights(sd, prefix)
    assert w.size == lib().tr_layer_weight_floats(d) and enc0.shape == (2, m, d // heads) and enc1.shape == (2, n, d // heads)
    out0, out1 = np.empty_like(desc0), np.empty_like(desc1)
    w0, w1 = _word(count0), _word(count1)
    rc = lib().tr_layer(_p(desc0), m, _p(desc1), n, d, heads, _p(enc0), _p(enc1), _p(w), _p(w0), _p(w1), int(variant), _p(out0), _p(out1))
    assert rc == 0
    return out0, out1


def same(a, b) -> bool:
    """Bit for bit, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _linear_weights(rng, outs, ins):
    """Seeded normals times 1 / sqrt(fan_in), and a small bias."""
    return ((rng.standard_normal((outs, ins)) / np.sqrt(ins)).astype(np.float32), (0.1 * rng.standard_normal(outs)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def state_dict(d, heads, n_layers, seed, d_in=None):
    """An upstream-style state dict of numpy arrays: ``n_layers`` transformer layers, posenc.Wr, the last layer's assignment head and,
    with ``d_in``, input_proj.  LayerNorm's weight is about 1 and its bias about 0, with noise."""
    rng = np.random.default_rng(seed)
    sd = {}
    for i in range(n_layers):
        for block, names in (("self_attn", (("Wqkv", 3 * d, d), ("out_proj", d, d))), ("cross_attn", (("to_qk", d, d), ("to_v", d, d), ("to_out", d, d)))):
            for name, outs, ins in names + (("ffn.0", 2 * d, 2 * d), ("ffn.3", d, 2 * d)):
                w, b = _linear_weights(rng, outs, ins)
                sd[f"transformers.{i}.{block}.{name}.weight"], sd[f"transformers.{i}.{block}.{name}.bias"] = w, b
            sd[f"transformers.{i}.{block}.ffn.1.weight"] = (1.0 + 0.1 * rng.standard_normal(2 * d)).astype(np.float32)
            sd[f"transformers.{i}.{block}.ffn.1.bias"] = (0.1 * rng.standard_normal(2 * d)).astype(np.float32)
    sd["posenc.Wr.weight"] = rng.standard_normal((d // heads // 2, 2)).astype(np.float32)
    head = f"log_assignment.{n_layers - 1}."
    sd[head + "final_proj.weight"] = (np.eye(d) + rng.standard_normal((d, d)) / np.sqrt(d) * 0.5).astype(np.float32)
    sd[head + "final_proj.bias"] = (0.1 * rng.standard_normal(d)).astype(np.float32)
    sd[head + "matchability.weight"] = (rng.standard_normal((1, d)) / np.sqrt(d)).astype(np.float32)
    sd[head + "matchability.bias"] = (0.5 * rng.standard_normal(1)).astype(np.float32)
    if d_in is not None:
        sd["input_proj.weight"], sd["input_proj.bias"] = _linear_weights(rng, d, d_in)
    _frozen(*sd.values())
    return sd


@functools.lru_cache(maxsize=None)
def inputs(m, n, d, heads, seed):
    """(desc0, desc1, kpts0, kpts1, size): unit descriptor rows, the second set's first rows a noisy permutation of the first's, and
    random keypoints in a 640 x 480 image."""
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((m, d)), rng.standard_normal((n, d))
    k = min(m, n)
    b[rng.permutation(k)] = a[:k] + 0.3 * rng.standard_normal((k, d))
    a /= np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-9)
    b /= np.maximum(np.linalg.norm(b, axis=1, keepdims=True), 1e-9)
    size = (640.0, 480.0)
    kp0 = (rng.random((m, 2)) * np.array(size)).astype(np.float32)
    kp1 = (rng.random((n, 2)) * np.array(size)).astype(np.float32)
    return _frozen(a.astype(np.float32), b.astype(np.float32), kp0, kp1) + (size,)


def encoding(kpts, size, Wr) -> np.ndarray:
    """``rotary_encoding`` in torch float32 on the CPU, the same ops as the package's: float32 [2, rows, dh].  (An input of the contract:
    the device's cos and sin may differ from the host's in the last bit, so the GPU tests upload THIS array.)"""
    import torch

    kpts, Wr = torch.from_numpy(np.array(kpts, np.float32)), torch.from_numpy(np.array(Wr, np.float32))
    size = torch.as_tensor(size, dtype=torch.float32)
    projected = ((kpts - size / 2) / (size.max() / 2)) @ Wr.t()
    return torch.stack([torch.cos(projected), torch.sin(projected)], 0).repeat_interleave(2, dim=-1).contiguous().numpy()


# (M, N, D, h, seed): the shapes of the layer's GPU tests.  One lane; partial 32-tiles and the non-vector path; a tile plus one and a
# key tile plus two with four heads; two column tiles of every Linear and dh = 64; the usual 300 keypoints.
LAYER_SHAPES = ((1, 1, 4, 2, 201), (33, 31, 8, 2, 202), (65, 130, 64, 4, 203), (130, 65, 256, 4, 204), (300, 300, 256, 4, 205))
# attention alone
ATTENTION_ROWS = ((1, 1), (31, 33), (33, 31), (64, 65), (65, 130), (130, 200))
ATTENTION_HEADS = ((2, 2), (4, 16), (1, 64), (4, 64))
# (M, N, h, dh): attention where the plan gives a wave 2 or 4 of a head's 32-column output tiles (at least 256 waves: ceil(M / 32) h), and
# head dimensions above 64 below that fill, whole tiles and a part of one, on the vector path and off it
ATTENTION_WIDE = ((1024, 130, 8, 64), (1024, 130, 8, 128), (1024, 70, 8, 66), (1024, 33, 8, 36), (65, 130, 2, 128), (33, 65, 3, 66), (64, 40, 1, 100))
# the layer where both of its attention launches run 2 output tiles a wave (32 row tiles x 4 heads x 2 sets, dh = 36)
LAYER_WIDE = (1024, 33, 144, 4, 206)


# (M, N, D, h, seed) with D % 4 != 0: every Linear of the layer runs its non-vector body and attention its scalar loads.  One lane and
# dh = 2; partial row tiles; dh = 10 in one head; dh = 6 and the key tile crossed in the cross block; D = 130: 3 D = 390 outputs are 4
# column tiles, the rotary boundary 2 D = 260 lies inside the third, and the second column tile of the D outputs holds 2 live columns
LAYER_NARROW = ((1, 1, 6, 3, 207), (33, 31, 6, 3, 208), (65, 34, 10, 1, 209), (40, 70, 18, 3, 210), (35, 33, 130, 5, 211))
# the Linear entry alone, (rows, in_dim, out_dim): a wave's 32 rows and a workgroup's 128 (transformer_plan.h's kLinearTileRows), the
# 32-column MFMA tiles and the 128-column tile of a workgroup, in_dim 1, odd and at the limit; every value of each list at least once
LINEAR_ROWS = (1, 31, 32, 33, 127, 128, 129)
LINEAR_INS = (1, 2, 3, 5, 8, 33, 100, 1024)
LINEAR_OUTS = (1, 31, 32, 33, 127, 128, 129, 1024)
LINEAR_CASES = ((1, 1, 1), (33, 1024, 129), (31, 2, 31), (32, 3, 32), (33, 5, 33), (127, 8, 127), (128, 33, 128), (129, 100, 129), (129, 1, 1024),
                (1, 1024, 1024), (32, 100, 1), (127, 33, 129), (128, 5, 127), (129, 3, 33), (31, 8, 128), (33, 2, 32))
LINEAR_HOSTILE = ((33, 5, 33), (33, 8, 33))
GELU_WEIGHT_SCALE = 6.0  # of both blocks' ffn.1.weight: |y / sqrt 2| reaches every branch of erf_c
HOSTILE_COUNTS = (3, 7)  # of hostile_layer_case: its bad rows lie behind them


def linear_tile_rows() -> int:
    """kLinearTileRows as csrc/transformer_plan.h states it (the text of the header; tests/test_transformer_args_cpu.py holds the plan's
    row tiles to it through the plan CLI)."""
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(_SRC)), "feature_tracker_amd", "csrc", "transformer_plan.h")).read()
    waves = int(re.search(r"constexpr int kLinearWaves = (\d+);", header).group(1))
    assert re.search(r"constexpr int kLinearTileRows = 32 \* kLinearWaves;", header)
    return 32 * waves


@functools.lru_cache(maxsize=None)
def linear_case(rows, ins, outs):
    """(x, weight, bias) of a Linear shape, seeded by the shape."""
    rng = np.random.default_rng(5000 + 1031 * rows + 17 * ins + outs)
    return _frozen(rng.standard_normal((rows, ins)).astype(np.float32), *_linear_weights(rng, outs, ins))


@functools.lru_cache(maxsize=None)
def hostile_linear_case(rows, ins, outs):
    """``linear_case`` with NaN, +-inf, -0 and subnormals scattered through x, weight and bias, and row 2 of x all +0 against a bias
    that is -0 at outputs 1 and 4: fmaf(+0, w, -0) is -0 for w < 0 and +0 for w > 0, and a k-step that added a +0 of its own would
    turn every such -0 into +0."""
    x, w, b = (np.array(a, copy=True) for a in linear_case(rows, ins, outs))
    x[0, 0], x[1, ins - 1], x[4, 1], x[5, 0], x[6, 2] = np.nan, np.inf, -np.inf, -0.0, 1e-40
    x[7] = -1e-41
    x[2] = 0.0
    w[0, 0], w[3, ins - 1], w[5, 1], w[6, 0], w[7] = np.inf, np.nan, -0.0, 1e-39, 3e-40
    w[1], w[4, :ins - 1], w[4, ins - 1] = -np.abs(w[1]), np.abs(w[4, :ins - 1]), -0.0  # row 2 of x: every product -0; +0 ... +0, -0
    b[1], b[4], b[8], b[9], b[10], b[11] = -0.0, -0.0, np.nan, np.inf, -np.inf, 1e-42
    return _frozen(x, w, b)


def scaled_gelu_case(shape, scale=GELU_WEIGHT_SCALE):
    """``layer_case`` with both blocks' LayerNorm weight times ``scale`` (a copy of the frozen state dict)."""
    a, b, e0, e1, sd = layer_case(shape)
    sd = dict(sd)
    for block in ("self_attn", "cross_attn"):
        key = f"transformers.0.{block}.ffn.1.weight"
        sd[key] = _frozen((sd[key] * np.float32(scale)).astype(np.float32))[0]
    return a, b, e0, e1, sd


def hostile_layer_case(shape):
    """``layer_case`` with bad rows behind HOSTILE_COUNTS, where attention masks them as keys and they spoil only themselves: a NaN, a
    row of zeros (variance 0) and a subnormal row in set 0; in set 1 a row of 1e30 (LayerNorm's sum of squares overflows: rstd = 0), a row
    of 3e38 (finite on input; the Linears' chains overflow and inf meets -inf: NaN) and a row that holds an inf."""
    a, b, e0, e1, sd = layer_case(shape)
    a, b = np.array(a, copy=True), np.array(b, copy=True)
    a[3, 5], a[11], a[12] = np.nan, 0.0, 1e-40
    b[7], b[8], b[9, 0] = 1e30, 3e38, np.inf
    assert min(3, 11, 12) >= HOSTILE_COUNTS[0] and min(7, 8, 9) >= HOSTILE_COUNTS[1]
    return _frozen(a, b) + (e0, e1, sd)


def self_block_hidden(x, heads, enc, sd, count=None, prefix="transformers.0.self_attn."):
    """The self block's rows in front of LayerNorm, ``ffn.0([x | message])``, composed from this module's exports: float32 [rows, 2 D]."""
    rows, d = x.shape
    dh = d // heads
    raw = linear(x, sd[prefix + "Wqkv.weight"], sd[prefix + "Wqkv.bias"]).reshape(rows, heads, dh, 3)  # upstream's (head, channel, q | k | v)
    q, k, v = (np.ascontiguousarray(raw[..., t]).reshape(rows, d) for t in range(3))
    q, k = rotary(q, heads, enc), rotary(k, heads, enc)
    ctx = attention(q.reshape(rows, heads, dh), k.reshape(rows, heads, dh), v.reshape(rows, heads, dh), count).reshape(rows, d)
    msg = linear(ctx, sd[prefix + "out_proj.weight"], sd[prefix + "out_proj.bias"])
    return linear(x, sd[prefix + "ffn.0.weight"], sd[prefix + "ffn.0.bias"], xb=msg)


def self_block_pre_gelu(x, heads, enc, sd, count=None, prefix="transformers.0.self_attn."):
    """The self block's values in front of GELU, ``LN(ffn.0([x | message])) gamma + beta``, with the LayerNorm in float64: float64
    [rows, 2 D].  For statements about the inputs of a test (which branch of erf_c a value takes), not for bit comparisons."""
    hid = self_block_hidden(x, heads, enc, sd, count, prefix).astype(np.float64)
    norm = (hid - hid.mean(1, keepdims=True)) / np.sqrt(hid.var(1, keepdims=True) + 1e-5)
    return norm * sd[prefix + "ffn.1.weight"].astype(np.float64) + sd[prefix + "ffn.1.bias"].astype(np.float64)


def erf_branch_shares(y):
    """The shares of a = |(float)y sqrt(1 / 2)| in erf_c's three branches: a < 1, 1 <= a < 4, a >= 4."""
    a = np.abs(np.asarray(y, np.float32) * np.float32(float.fromhex("0x1.6a09e6p-1"))).ravel()  # the kernel's product, in float32
    return float((a < 1).mean()), float(((a >= 1) & (a < 4)).mean()), float((a >= 4).mean())


@functools.lru_cache(maxsize=None)
def qkv(m, n, h, dh, seed):
    rng = np.random.default_rng(seed)
    return _frozen(rng.standard_normal((m, h, dh)).astype(np.float32), rng.standard_normal((n, h, dh)).astype(np.float32),
                   rng.standard_normal((n, h, dh)).astype(np.float32))


def layer_case(shape):
    """(desc0, desc1, enc0, enc1, sd) of a layer shape."""
    m, n, d, h, seed = shape
    sd = state_dict(d, h, 1, seed + 1000)
    a, b, kp0, kp1, size = inputs(m, n, d, h, seed)
    return a, b, encoding(kp0, size, sd["posenc.Wr.weight"]), encoding(kp1, size, sd["posenc.Wr.weight"]), sd
