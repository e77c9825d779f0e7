"""ctypes binding of tests/flow_warm_ref.c — the scalar CPU restatement of the warm start of RAFT on video.

TEST INFRASTRUCTURE ONLY: compiled on first use (gcc -O3 -ffp-contract=off, plus -mfma where the CPU has it so that fmaf is one
instruction instead of a libm call — the same correctly rounded operation either way) into a temporary directory; nothing under
feature_tracker_amd/ may import it, and it imports nothing from there.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests.flow_points_ref import same  # noqa: F401  (same: bit-identical arrays, any NaN equals any NaN)
from tests.ref_build import FMA, STRICT, compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "flow_warm_ref.c")

CONTRACT, MUTANT_HIGHEST_INDEX, MUTANT_CLOSED_BOUNDS, MUTANT_SWAPPED_XY = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("flow_warm_ref", [_SRC], flags=STRICT + FMA)  # -mfma where the CPU has it: fmaf as one instruction (see above)
    vp, i32 = C.c_void_p, C.c_int32
    l.fwr_warm.argtypes = [vp, i32, i32, i32, i32, vp, vp]
    l.fwr_warm.restype = i32
    return l


def warm(flow, variant: int = CONTRACT, with_chosen: bool = False):
    """flow [B, 2, H, W] -> the warm start [B, 2, H, W]; with_chosen: and the winning source index of each target [B, H, W] int32
    (y * W + x, -1 in an entry without a valid source)."""
    flow = np.ascontiguousarray(flow, dtype=np.float32)
    B, two, H, W = flow.shape
    assert two == 2
    out = np.empty_like(flow)
    chosen = np.empty((B, H, W), np.int32)
    rc = lib().fwr_warm(flow.ctypes.data_as(C.c_void_p), B, H, W, int(variant), out.ctypes.data_as(C.c_void_p), chosen.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return (out, chosen) if with_chosen else out
