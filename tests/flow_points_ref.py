"""ctypes binding of tests/flow_points_ref.c — the scalar CPU restatement of sparse tracking from RAFT's coarse flow.

TEST INFRASTRUCTURE ONLY: compiled on first use (gcc -O3 -ffp-contract=off, plus -mfma where the CPU has it so that fmaf is one
instruction instead of a libm call — the same correctly rounded operation either way) into a temporary directory; nothing under
feature_tracker_amd/ may import it, and it imports nothing from there.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests.ref_build import FMA, STRICT, compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "flow_points_ref.c")

CONTRACT, MUTANT_SWAPPED_UV, MUTANT_WRAPPED_NEIGHBOUR = 0, 1, 2
NOT_TRACKED, TRACKED, LARGE_RESIDUAL, OUTSIDE, NUMERIC_ERROR = 0, 1, 2, 3, 4  # include/ftk.h's TrackStatus


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("flow_points_ref", [_SRC], flags=STRICT + FMA)  # -mfma where the CPU has it: fmaf as one instruction (see above)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    l.fpr_bilinear.argtypes = [f32] * 6
    l.fpr_bilinear.restype = f32
    l.fpr_bilinear_array.argtypes = [vp] * 6 + [i64, vp]
    l.fpr_bilinear_array.restype = None
    l.fpr_track.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, f32, i32, vp, vp, vp, vp]
    l.fpr_track.restype = i32
    l.fpr_track_dense.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, f32, i32, vp, vp, vp, vp]
    l.fpr_track_dense.restype = i32
    return l


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def bilinear(v00, v01, v10, v11, fx, fy):
    """The contract's three fmaf, element by element over float32 arrays of one shape."""
    args = [_f32(a) for a in np.broadcast_arrays(v00, v01, v10, v11, fx, fy)]
    out = np.empty_like(args[0])
    lib().fpr_bilinear_array(*[_p(a) for a in args], out.size, _p(out))
    return out


def _outputs(B, N, with_error):
    return np.empty((B, N, 2), np.float32), np.empty((B, N), np.uint8), (np.empty((B, N), np.float32) if with_error else None)


def track(flow, mask, points, image_size, mask_scale: float = 1.0, backward=None, fb_threshold: float = 0.0, variant: int = CONTRACT):
    """flow [B, 2, H, W], mask [B, 576, H, W], points [B, N, 2], image_size (rows, cols), backward (flow_back, mask_back) or None ->
    (cur_points [B, N, 2], status [B, N] uint8, fb_error2 [B, N] or None without the backward pair)."""
    flow, mask, points = _f32(flow), _f32(mask), _f32(points)
    B, two, H, W = flow.shape
    N = points.shape[1]
    assert two == 2 and mask.shape == (B, 576, H, W) and points.shape == (B, N, 2)
    fb, mb = (None, None) if backward is None else (_f32(backward[0]), _f32(backward[1]))
    assert backward is None or (fb.shape == flow.shape and mb.shape == mask.shape)
    cur, status, err = _outputs(B, N, backward is not None)
    rc = lib().fpr_track(_p(flow), _p(mask), _p(fb), _p(mb), B, H, W, N, int(image_size[0]), int(image_size[1]), float(mask_scale), float(fb_threshold),
                         int(variant), _p(points), _p(cur), _p(status), _p(err))
    assert rc == 0
    return cur, status, err


def track_dense(dense, points, image_size, dense_back=None, fb_threshold: float = 0.0, variant: int = CONTRACT):
    """The same rules on stored fine fields [B, 2, 8H, 8W] (upsample_flow's output), dense_back or None."""
    dense, points = _f32(dense), _f32(points)
    B, two, H8, W8 = dense.shape
    N = points.shape[1]
    assert two == 2 and H8 % 8 == 0 and W8 % 8 == 0 and points.shape == (B, N, 2)
    back = None if dense_back is None else _f32(dense_back)
    assert back is None or back.shape == dense.shape
    cur, status, err = _outputs(B, N, back is not None)
    rc = lib().fpr_track_dense(_p(dense), _p(back), B, H8 // 8, W8 // 8, N, int(image_size[0]), int(image_size[1]), float(fb_threshold), int(variant),
                               _p(points), _p(cur), _p(status), _p(err))
    assert rc == 0
    return cur, status, err


def same(a, b) -> bool:
    """Bit-identical arrays, except that any NaN equals any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
