"""ctypes binding of tests/raft_encoder_ref.c — the scalar CPU restatement of the layers of RAFT's encoders — and the
networks composed from it and from the other restatements: ``feature_encoder`` / ``context_encoder`` (encoder.py:25-68) and ``raft``
(model.py:66-97: the correlation pyramid of tests/raft_corr_ref, the update block of tests/raft_conv_ref, the upsampling of
tests/flow_upsample_ref, and the three float32 element-wise operations of model.py:90-94 in numpy, which rounds them once each).

TEST INFRASTRUCTURE ONLY: compiled on first use exactly as raft_conv_ref.py does it (gcc -O3 -ffp-contract=off, plus -mfma where the
CPU has it) together with raft_conv_ref.c and sep_conv_gru_ref.c, into a temporary directory; nothing under feature_tracker_amd/ may
import it.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests import flow_upsample_ref, raft_conv_ref, raft_corr_ref
from tests.flow_upsample_ref import same  # noqa: F401  (same: bit-identical, any NaN equals any NaN)
from tests.ref_build import FMA, STRICT, compile_ref

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRCS = [os.path.join(_HERE, f) for f in ("raft_encoder_ref.c", "raft_conv_ref.c", "sep_conv_gru_ref.c")]

BN_EPS = np.float32(1e-5)
(CONTRACT, MUTANT_STRIDE_TAP_WITHOUT_PAD, MUTANT_OUTPUT_SIZE_FLOOR, MUTANT_FOLD_WITHOUT_SQRT, MUTANT_FOLD_WITHOUT_EPS, MUTANT_RESIDUAL_AFTER_RELU,
 MUTANT_SHORTCUT_BN_SKIPPED, MUTANT_NORMALISATION_DROPPED, MUTANT_PADDING_NORMALISED, MUTANT_REF_PLUS_DELTA) = range(10)
MUTANTS = {"stride tap without - pad": MUTANT_STRIDE_TAP_WITHOUT_PAD, "output size floor(H / 2)": MUTANT_OUTPUT_SIZE_FLOOR,
           "var + eps without the square root": MUTANT_FOLD_WITHOUT_SQRT, "eps dropped": MUTANT_FOLD_WITHOUT_EPS,
           "residual added after the ReLU": MUTANT_RESIDUAL_AFTER_RELU, "the shortcut's BatchNorm skipped": MUTANT_SHORTCUT_BN_SKIPPED,
           "normalisation dropped": MUTANT_NORMALISATION_DROPPED, "padding normalised to -1": MUTANT_PADDING_NORMALISED,
           "ref + delta instead of cur + delta": MUTANT_REF_PLUS_DELTA}
BLOCKS = tuple((f"resnet_{k}.{i}", 1 + i) for k in (1, 2, 3) for i in (0, 1))  # (name, stride): encoder.py:33-44
BN_KINDS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("raft_encoder_ref", _SRCS, flags=STRICT + FMA)  # -mfma where the CPU has it: fmaf as one instruction (see above)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    l.re_normalise.argtypes, l.re_normalise.restype = [f32], f32
    l.re_fold.argtypes, l.re_fold.restype = [vp, vp, vp, vp, vp, f32, i32, i64, i32, vp, vp], i32
    l.re_conv2d.argtypes, l.re_conv2d.restype = [vp, i32, vp, vp, i32, i32, i32, vp, i32, f32, i32, i32, i32, i32, i32, vp], i32
    return l


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)


def normalise(x):
    """model.py:70-71 on a float32 array, element by element through the C function."""
    x = _f32(x)
    return np.array([lib().re_normalise(float(v)) for v in x.ravel()], np.float32).reshape(x.shape)


def fold(weight, gamma, beta, mean, var, eps=BN_EPS, variant: int = CONTRACT):
    """A bias-free convolution [Cout, Cin, ks, ks] and the BatchNorm (eval mode) after it as (w', b')."""
    weight, gamma, beta, mean, var = (_f32(t) for t in (weight, gamma, beta, mean, var))
    M = weight.shape[0]
    assert all(t.shape == (M,) for t in (gamma, beta, mean, var))
    w, b = np.empty_like(weight), np.empty(M, np.float32)
    rc = lib().re_fold(_p(weight), _p(gamma), _p(beta), _p(mean), _p(var), float(eps), M, weight.size // M, int(variant), _p(w), _p(b))
    assert rc == 0, rc
    return w, b


def fold_numpy(weight, gamma, beta, mean, var, eps=BN_EPS):
    """The same fold in numpy float32: division and square root are correctly rounded, so this is bit-equal to the C one."""
    weight, gamma, beta, mean, var = (_f32(t) for t in (weight, gamma, beta, mean, var))
    s = gamma / np.sqrt(var + np.float32(eps))
    return weight * s[:, None, None, None], beta - mean * s


def out_size(n: int, stride: int) -> int:
    return -(-n // stride)


def conv2d(x, weight, bias, stride: int = 1, residual=None, relu: bool = False, scale: float = 1.0, normalise: bool = False,
           variant: int = CONTRACT):
    """x float32 [B, Cin, H, W]; weight [Cout, Cin, ks, ks]; bias [Cout]; residual None or of the output's shape -> [B, Cout, ceil(H / S),
    ceil(W / S)]."""
    x, weight, bias = _f32(x), _f32(weight), _f32(bias)
    B, Cin, H, W = x.shape
    Cout, Cin2, ks, ks2 = weight.shape
    assert ks == ks2 and Cin == Cin2 and bias.shape == (Cout,), (x.shape, weight.shape, bias.shape)
    out = np.empty((B, Cout, out_size(H, stride), out_size(W, stride)), np.float32)
    if residual is not None:
        residual = _f32(residual)
        assert residual.shape == out.shape, (residual.shape, out.shape)
    rc = lib().re_conv2d(_p(x), Cin, _p(weight), _p(bias), Cout, ks, int(stride), _p(residual), int(bool(relu)), float(scale), int(bool(normalise)),
                         B, H, W, int(variant), _p(out))
    assert rc == 0, rc
    return out


def encoder_keys(prefix, shortcuts=(False, True, False, True, False, True)):
    """The key names of a FeatureEncoder's state dict (encoder.py:25-48)."""
    keys = [f"{prefix}conv_in.0.weight", f"{prefix}conv_in.0.bias"]
    for (name, _), shortcut in zip(BLOCKS, shortcuts):
        for conv, bn in (("conv1", "bn1"), ("conv2", "bn2")) + ((("shortcut.0", "shortcut.1"),) if shortcut else ()):
            keys.append(f"{prefix}{name}.{conv}.weight")
            keys += [f"{prefix}{name}.{bn}.{kind}" for kind in BN_KINDS]
    return keys + [f"{prefix}conv_out.0.weight", f"{prefix}conv_out.0.bias"]


def feature_encoder(image, state, prefix: str = "", normalise_image: bool = False, variant: int = CONTRACT, eps=BN_EPS):
    """encoder.py:49-55 over ``state`` (a mapping of arrays or tensors under the module's names): 17 layers.  A mutant of the output size
    crops every stride-2 layer's output to floor(H / 2) x floor(W / 2)."""
    g = lambda k: _f32(state[prefix + k])  # noqa: E731
    cv = variant if variant in (MUTANT_STRIDE_TAP_WITHOUT_PAD, MUTANT_RESIDUAL_AFTER_RELU, MUTANT_PADDING_NORMALISED) else CONTRACT
    fv = variant if variant in (MUTANT_FOLD_WITHOUT_SQRT, MUTANT_FOLD_WITHOUT_EPS) else CONTRACT

    def folded(conv, bn, skip_bn=False):
        w = g(conv + ".weight")
        if skip_bn:
            return w, np.zeros(w.shape[0], np.float32)
        return fold(w, g(bn + ".weight"), g(bn + ".bias"), g(bn + ".running_mean"), g(bn + ".running_var"), eps, fv)

    def strided(x, w, b, stride, **kw):
        out = conv2d(x, w, b, stride, variant=cv, **kw)
        if variant == MUTANT_OUTPUT_SIZE_FLOOR and stride == 2:
            out = np.ascontiguousarray(out[:, :, :x.shape[2] // 2, :x.shape[3] // 2])
        return out

    x = strided(image, g("conv_in.0.weight"), g("conv_in.0.bias"), 1, relu=True, normalise=normalise_image and variant != MUTANT_NORMALISATION_DROPPED)
    for name, stride in BLOCKS:
        t = strided(x, *folded(f"{name}.conv1", f"{name}.bn1"), stride, relu=True)
        r = x
        if f"{prefix}{name}.shortcut.0.weight" in state:
            r = strided(x, *folded(f"{name}.shortcut.0", f"{name}.shortcut.1", variant == MUTANT_SHORTCUT_BN_SKIPPED), stride)
        if 0 in t.shape:
            return t
        x = strided(t, *folded(f"{name}.conv2", f"{name}.bn2"), 1, residual=r, relu=True)
    return strided(x, g("conv_out.0.weight"), g("conv_out.0.bias"), 1, relu=True)


def context_encoder(image, state, prefix: str, context_channels: int, normalise_image: bool = False, variant: int = CONTRACT):
    """encoder.py:64-68: (context, hidden), each contiguous."""
    x = feature_encoder(image, state, prefix + "net.", normalise_image, variant)
    return np.ascontiguousarray(x[:, :context_channels]), np.ascontiguousarray(x[:, context_channels:])


def raft(ref_image, cur_image, state, levels: int, radius: int, iterations: int, variant: int = CONTRACT):
    """model.py:66-97 over a whole model's ``state``: the list of predictions [B, 2, 8h, 8w]."""
    ref_image, cur_image = _f32(ref_image), _f32(cur_image)
    B = ref_image.shape[0]
    features = feature_encoder(np.concatenate([ref_image, cur_image], 0), state, "feature_encoder.", True, variant)
    block = raft_conv_ref.weights_of(state, "update_block.")
    net_channels = block["flow_head.conv1.weight"].shape[1]
    total = _f32(state["context_encoder.net.conv_out.0.weight"]).shape[0]
    if 0 in features.shape:
        return None
    pyramid = raft_corr_ref.build(features[:B], features[B:], levels)
    inp, net = context_encoder(ref_image, state, "context_encoder.", total - net_channels, True, variant)
    h, w = features.shape[2:]
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    ref = np.ascontiguousarray(np.broadcast_to(np.stack([xs, ys])[None], (B, 2, h, w)))
    cur = ref
    predictions = []
    for _ in range(iterations):
        correlation = raft_corr_ref.lookup(pyramid, cur, radius)
        flow = cur - ref
        net, mask, delta = raft_conv_ref.update_block(net, inp, correlation, flow, block)[:3]
        cur = (ref if variant == MUTANT_REF_PLUS_DELTA else cur) + delta
        predictions.append(flow_upsample_ref.upsample(cur - ref, mask))
    return predictions
