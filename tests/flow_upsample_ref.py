"""ctypes binding of tests/flow_upsample_ref.c — the scalar CPU restatement of RAFT's convex flow upsampling.

TEST INFRASTRUCTURE ONLY: compiled on first use (gcc -O3 -ffp-contract=off, plus -mfma where the CPU has it so that fmaf is one
instruction instead of a libm call — the same correctly rounded operation either way) into a temporary directory; nothing under
feature_tracker_amd/ may import it.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests.ref_build import FMA, STRICT, compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "flow_upsample_ref.c")

CONTRACT, MUTANT_TRANSPOSED_WINDOW, MUTANT_DEGREE_3 = 0, 1, 2


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("flow_upsample_ref", [_SRC], flags=STRICT + FMA)  # -mfma where the CPU has it: fmaf as one instruction (see above)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    l.fur_exp_c.argtypes = [f32]
    l.fur_exp_c.restype = f32
    l.fur_exp_c_array.argtypes = [vp, i64, vp]
    l.fur_exp_c_array.restype = None
    l.fur_cutoff.argtypes = []
    l.fur_cutoff.restype = f32
    l.fur_upsample.argtypes = [vp, vp, i32, i32, i32, f32, i32, vp]
    l.fur_upsample.restype = i32
    return l


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def cutoff() -> np.float32:
    return np.float32(lib().fur_cutoff())


def exp_c(t):
    """exp_c of a float32 array, element by element."""
    t = np.ascontiguousarray(t, dtype=np.float32)
    out = np.empty_like(t)
    lib().fur_exp_c_array(_p(t), t.size, _p(out))
    return out


def upsample(flow, mask, mask_scale: float = 1.0, variant: int = CONTRACT):
    """flow float32 [B, 2, H, W], mask float32 [B, 576, H, W] -> [B, 2, 8H, 8W]."""
    flow = np.ascontiguousarray(flow, dtype=np.float32)
    mask = np.ascontiguousarray(mask, dtype=np.float32)
    B, two, H, W = flow.shape
    assert two == 2 and mask.shape == (B, 576, H, W)
    out = np.empty((B, 2, 8 * H, 8 * W), np.float32)
    rc = lib().fur_upsample(_p(flow), _p(mask), B, H, W, float(mask_scale), int(variant), _p(out))
    assert rc == 0
    return out


def same(a, b) -> bool:
    """Bit-identical float arrays, except that any NaN equals any NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
