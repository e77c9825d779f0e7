"""ctypes binding of tests/sep_conv_gru_ref.c — the scalar CPU restatement of RAFT's separable ConvGRU.

TEST INFRASTRUCTURE ONLY: compiled on first use (gcc -O3 -ffp-contract=off, plus -mfma where the CPU has it so that fmaf is one
instruction instead of a libm call — the same correctly rounded operation either way) into a temporary directory; nothing under
feature_tracker_amd/ may import it.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests.flow_upsample_ref import same  # noqa: F401  (same: bit-identical, any NaN equals any NaN)
from tests.ref_build import FMA, STRICT, compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sep_conv_gru_ref.c")

CONTRACT, MUTANT_TAPS_REVERSED, MUTANT_Z_R_EXCHANGED, MUTANT_VERTICAL_FIRST, MUTANT_BLEND_EXCHANGED, MUTANT_CLAMPED_PADDING = range(6)
MUTANTS = {"taps reversed": MUTANT_TAPS_REVERSED, "z and r weights exchanged": MUTANT_Z_R_EXCHANGED, "vertical pass first": MUTANT_VERTICAL_FIRST,
           "z and 1 - z exchanged": MUTANT_BLEND_EXCHANGED, "clamped padding": MUTANT_CLAMPED_PADDING}
# the reference module's parameter names, in the order scg_forward takes them
GATES = ("z_horizontal", "r_horizontal", "q_horizontal", "z_vertical", "r_vertical", "q_vertical")


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("sep_conv_gru_ref", [_SRC], flags=STRICT + FMA)  # -mfma where the CPU has it: fmaf as one instruction (see above)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    for name in ("scg_sigmoid_c", "scg_tanh_c"):
        getattr(l, name).argtypes = [f32]
        getattr(l, name).restype = f32
        getattr(l, name + "_array").argtypes = [vp, i64, vp]
        getattr(l, name + "_array").restype = None
    l.scg_tanh_small.argtypes = []
    l.scg_tanh_small.restype = f32
    l.scg_forward.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    l.scg_forward.restype = i32
    return l


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _elementwise(name, v):
    v = np.ascontiguousarray(v, dtype=np.float32)
    out = np.empty_like(v)
    getattr(lib(), name)(_p(v), v.size, _p(out))
    return out


def sigmoid_c(v):
    return _elementwise("scg_sigmoid_c_array", v)


def tanh_c(v):
    return _elementwise("scg_tanh_c_array", v)


def tanh_small() -> np.float32:
    return np.float32(lib().scg_tanh_small())


def weights_of(state, prefix=""):
    """The twelve arrays of a state dict of the reference's SepConvGru (torch tensors or arrays), as float32 numpy arrays."""
    out = {}
    for g in GATES:
        for kind in ("weight", "bias"):
            t = state[f"{prefix}conv_{g}.{kind}"]
            out[f"conv_{g}.{kind}"] = np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)
    return out


def forward(x, h, state, variant: int = CONTRACT):
    """x: one float32 array [B, Cx, H, W] or a sequence of parts; h [B, Ch, H, W]; state: weights_of(...) -> the new h."""
    parts = [x] if isinstance(x, np.ndarray) else list(x)
    parts = [np.ascontiguousarray(p, dtype=np.float32) for p in parts]
    h = np.ascontiguousarray(h, dtype=np.float32)
    B, Ch, H, W = h.shape
    Cx = sum(p.shape[1] for p in parts)
    w = [state[f"conv_{g}.weight"] for g in GATES]
    b = [state[f"conv_{g}.bias"] for g in GATES]
    ks = max(w[0].shape[2], w[0].shape[3])
    for k, wk in enumerate(w):
        assert wk.shape == ((Ch, Cx + Ch, 1, ks) if k < 3 else (Ch, Cx + Ch, ks, 1)) and b[k].shape == (Ch,), (k, wk.shape)
    assert all(p.shape == (B, p.shape[1], H, W) for p in parts)
    part_ptrs = (C.c_void_p * len(parts))(*[p.ctypes.data for p in parts])
    part_channels = (C.c_int32 * len(parts))(*[p.shape[1] for p in parts])
    w_ptrs = (C.c_void_p * 6)(*[a.ctypes.data for a in w])
    b_ptrs = (C.c_void_p * 6)(*[a.ctypes.data for a in b])
    out = np.empty_like(h)
    rc = lib().scg_forward(part_ptrs, part_channels, len(parts), _p(h), w_ptrs, b_ptrs, Ch, ks, B, H, W, int(variant), _p(out))
    assert rc == 0, rc
    return out
