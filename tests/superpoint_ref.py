"""ctypes binding of tests/superpoint_ref.c — the scalar CPU restatement of the pooled conv layer and of the dense descriptor
normalisation — and SuperPoint's network composed from it and from tests/raft_conv_ref's layer, over upstream-style
unpacked tensors (``conv1a`` ... ``convDb``, ``.weight`` / ``.bias``).

TEST INFRASTRUCTURE ONLY: compiled on first use exactly as raft_conv_ref.py does it (gcc -O3 -ffp-contract=off, plus -mfma where the CPU
has it) together with raft_conv_ref.c and sep_conv_gru_ref.c, into a temporary directory; nothing under feature_tracker_amd/ may import it.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests import raft_conv_ref
from tests.flow_upsample_ref import same  # noqa: F401  (same: bit-identical, any NaN equals any NaN)
from tests.ref_build import FMA, STRICT, compile_ref

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRCS = [os.path.join(_HERE, f) for f in ("superpoint_ref.c", "raft_conv_ref.c", "sep_conv_gru_ref.c")]

CONTRACT, MUTANT_POOL_SHIFTED, MUTANT_POOL_FMAXF, MUTANT_NO_FLOOR, MUTANT_HEADS_EXCHANGED = range(5)
MUTANTS = {"pooling window shifted by one pixel": MUTANT_POOL_SHIFTED, "pool as fmaxf of the four": MUTANT_POOL_FMAXF,
           "normalisation without the 1e-12 floor": MUTANT_NO_FLOOR, "the two heads' halves exchanged": MUTANT_HEADS_EXCHANGED}
LAYERS = ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPa", "convPb", "convDa", "convDb")
POOLED = ("conv1b", "conv2b", "conv3b")


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("superpoint_ref", _SRCS, flags=STRICT + FMA)  # -mfma where the CPU has it: fmaf as one instruction (see above)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    l.sp_max_pool.argtypes, l.sp_max_pool.restype = [vp, i64, i32, i32, i32, vp], i32
    l.sp_conv2d_pool.argtypes, l.sp_conv2d_pool.restype = [vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp], i32
    l.sp_channel_normalise.argtypes, l.sp_channel_normalise.restype = [vp, i32, i64, i32, vp], i32
    return l


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)


def max_pool(x, variant: int = CONTRACT):
    """float32 [..., H, W] -> [..., H // 2, W // 2]."""
    x = _f32(x)
    H, W = x.shape[-2:]
    out = np.empty(x.shape[:-2] + (H // 2, W // 2), np.float32)
    rc = lib().sp_max_pool(_p(x), int(np.prod(x.shape[:-2], dtype=np.int64)), H, W, int(variant), _p(out))
    assert rc == 0, rc
    return out


def conv2d_pool(parts, weight, bias, relu: bool, variant: int = CONTRACT, return_pre: bool = False):
    """parts: one float32 array [B, C, H, W] or a sequence of them; weight [Cout, Cin, ks, ks]; bias [Cout] -> [B, Cout, H // 2, W // 2]
    (and, with ``return_pre``, the restatement's own tensor before the pool, [B, Cout, H, W])."""
    parts = [parts] if isinstance(parts, np.ndarray) else list(parts)
    parts = [_f32(p) for p in parts]
    weight, bias = _f32(weight), _f32(bias)
    B, _, H, W = parts[0].shape
    Cout, Cin, ks, ks2 = weight.shape
    assert ks == ks2 and bias.shape == (Cout,) and sum(p.shape[1] for p in parts) == Cin, (weight.shape, bias.shape, [p.shape for p in parts])
    assert all(p.shape == (B, p.shape[1], H, W) for p in parts)
    ptrs = (C.c_void_p * len(parts))(*[p.ctypes.data for p in parts])
    channels = (C.c_int32 * len(parts))(*[p.shape[1] for p in parts])
    out = np.empty((B, Cout, H // 2, W // 2), np.float32)
    pre = np.empty((B, Cout, H, W), np.float32) if return_pre else None
    rc = lib().sp_conv2d_pool(ptrs, channels, len(parts), _p(weight), _p(bias), Cout, ks, int(bool(relu)), B, H, W, int(variant), _p(pre), _p(out))
    assert rc == 0, rc
    return (out, pre) if return_pre else out


def channel_normalise(x, variant: int = CONTRACT):
    """float32 [D, Hc, Wc] -> [Hc, Wc, D], every cell of unit length."""
    x = _f32(x)
    D, hc, wc = x.shape
    y = np.empty((hc, wc, D), np.float32)
    rc = lib().sp_channel_normalise(_p(x), D, hc * wc, int(variant), _p(y))
    assert rc == 0, rc
    return y


def weights_of(state, prefix=""):
    return {f"{layer}.{kind}": _f32(state[f"{prefix}{layer}.{kind}"]) for layer in LAYERS for kind in ("weight", "bias")}


def heads(image, state, variant: int = CONTRACT):
    """Upstream's forward pass up to the two head tensors on a float32 image [H, W]: (semi [65, Hc, Wc], desc [D, Hc, Wc] as the
    transposed view of the normalised [Hc, Wc, D])."""
    image = _f32(image)
    x = image.reshape(1, 1, *image.shape[-2:])
    pool_variant = variant if variant in (MUTANT_POOL_SHIFTED, MUTANT_POOL_FMAXF) else CONTRACT
    for layer in LAYERS[:8]:
        w, b = state[layer + ".weight"], state[layer + ".bias"]
        x = conv2d_pool(x, w, b, True, pool_variant) if layer in POOLED else raft_conv_ref.conv2d(x, w, b, True)
    c_pa = raft_conv_ref.conv2d(x, state["convPa.weight"], state["convPa.bias"], True)
    c_da = raft_conv_ref.conv2d(x, state["convDa.weight"], state["convDa.bias"], True)
    if variant == MUTANT_HEADS_EXCHANGED:  # the stacked tensor read as [convDa | convPa]
        both = np.concatenate([c_pa, c_da], 1)
        c_pa, c_da = np.ascontiguousarray(both[:, both.shape[1] - c_pa.shape[1]:]), np.ascontiguousarray(both[:, :c_da.shape[1]])
    semi = raft_conv_ref.conv2d(c_pa, state["convPb.weight"], state["convPb.bias"], False)[0]
    dmap = raft_conv_ref.conv2d(c_da, state["convDb.weight"], state["convDb.bias"], False)[0]
    normal = channel_normalise(dmap, variant if variant == MUTANT_NO_FLOOR else CONTRACT)
    return semi, np.transpose(normal, (2, 0, 1))


def make_state(widths, seed: int):
    """torch.nn.Conv2d's own default initialisation of upstream's twelve layers; ``widths`` = (c1, c2, c3, c4, head, D)."""
    import torch
    c1, c2, c3, c4, head, d = widths
    shapes = {"conv1a": (c1, 1, 3), "conv1b": (c1, c1, 3), "conv2a": (c2, c1, 3), "conv2b": (c2, c2, 3), "conv3a": (c3, c2, 3), "conv3b": (c3, c3, 3),
              "conv4a": (c4, c3, 3), "conv4b": (c4, c4, 3), "convPa": (head, c4, 3), "convPb": (65, head, 1), "convDa": (head, c4, 3), "convDb": (d, head, 1)}
    torch.manual_seed(300 + seed)
    state = {}
    for name, (M, Cin, ks) in shapes.items():
        conv = torch.nn.Conv2d(Cin, M, ks, stride=1, padding=ks // 2)
        state[name + ".weight"], state[name + ".bias"] = conv.weight.detach().clone(), conv.bias.detach().clone()
    return state


def make_image(H, W, seed: int):
    """A float32 image in 0 .. 1."""
    return np.random.default_rng(400 + seed).uniform(0.0, 1.0, (H, W)).astype(np.float32)


def hostile_pool_image():
    """An 8 x 16 image of 32 pooling windows: for each position of a window in turn, the value that decides the window placed there: a NaN
    among finite values, +inf among finite values, one finite value among -inf, -0 among +0 and +0 among -0 (equal: the first of the scan
    stays), and a subnormal among zeros; the last eight windows are ordinary values."""
    rng = np.random.default_rng(77)
    image = rng.standard_normal((8, 16)).astype(np.float32)
    sub = np.float32(1e-45)
    kinds = ((np.nan, None), (np.inf, None), (np.float32(-3.5), -np.inf), (np.float32(-0.0), np.float32(0.0)), (np.float32(0.0), np.float32(-0.0)), (sub, np.float32(0.0)))
    for k, (special, others) in enumerate(kinds):
        for p in range(4):
            n = 4 * k + p
            wy, wx = 2 * (n // 8), 2 * (n % 8)
            if others is not None:
                image[wy:wy + 2, wx:wx + 2] = others
            image[wy + p // 2, wx + p % 2] = special
    image.setflags(write=False)
    return image
