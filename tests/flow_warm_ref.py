"""ctypes binding of tests/flow_warm_ref.c — the scalar CPU restatement of the warm start of RAFT on video.

TEST INFRASTRUCTURE ONLY: compiled on first use (gcc -O3 -ffp-contract=off, plus -mfma where the CPU has it so that fmaf is one
instruction instead of a libm call — the same correctly rounded operation either way) into a temporary directory; nothing under
feature_tracker_amd/ may import it, and it imports nothing from there.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests.flow_points_ref import _cpu_has_fma, same  # noqa: F401  (same: bit-identical arrays, any NaN equals any NaN)

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "flow_warm_ref.c")
_lib = None
_tmpdir = None

CONTRACT, MUTANT_HIGHEST_INDEX, MUTANT_CLOSED_BOUNDS, MUTANT_SWAPPED_XY = 0, 1, 2, 3


def lib():
    global _lib, _tmpdir
    if _lib is None:
        _tmpdir = tempfile.TemporaryDirectory(prefix="flow_warm_ref_")
        path = os.path.join(_tmpdir.name, "libflow_warm_ref.so")
        flags = ["-O3", "-std=c99", "-ffp-contract=off", "-fno-fast-math"] + (["-mfma"] if _cpu_has_fma() else [])
        subprocess.run(["gcc"] + flags + ["-shared", "-fPIC", "-o", path, _SRC, "-lm"], check=True, capture_output=True)
        l = C.CDLL(path)
        vp, i32 = C.c_void_p, C.c_int32
        l.fwr_warm.argtypes = [vp, i32, i32, i32, i32, vp, vp]
        l.fwr_warm.restype = i32
        _lib = l
    return _lib


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
