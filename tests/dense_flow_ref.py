"""ctypes binding of tests/dense_flow_ref.c — the scalar CPU restatement of DenseOpticalFlow (Farneback).

TEST INFRASTRUCTURE ONLY: compiled on first use with the oracle's flags (gcc -O3 -ffp-contract=off) into a temporary
directory; nothing under feature_tracker_amd/ may import it.

The restatement is pinned independently by ref64 (tests/dense_ref64.py): tests/test_dense_ref64_cpu.py compares it with that float64
restatement stage by stage and end to end; tests/test_dense_ref64_gpu.py compares the kernels with ref64 directly.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests.ref_build import compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dense_flow_ref.c")


class Options(C.Structure):
    _fields_ = [("max_iteration", C.c_int32), ("half_patch", C.c_int32), ("max_converge_step", C.c_float), ("max_delta_flow_step", C.c_float)]


def options(max_iteration=10, half_patch=2, max_converge_step=1e-6, max_delta_flow_step=1.0) -> Options:
    """DenseOpticalFlow::Options (dense_optical_flow.h:15-20), same defaults."""
    return Options(int(max_iteration), int(half_patch), float(max_converge_step), float(max_delta_flow_step))


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("dense_flow_ref", [_SRC])
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    l.dfr_interpolate.argtypes = [vp, i32, i32, f32, f32]
    l.dfr_interpolate.restype = f32
    l.dfr_median9.argtypes = [vp]
    l.dfr_median9.restype = f32
    l.dfr_gaussian.argtypes = [i32, vp, vp]
    l.dfr_moments_f32.argtypes = [vp, i32, i32, i32, vp, vp]
    l.dfr_moments_u8.argtypes = [vp, i32, i32, i32, vp, vp]
    l.dfr_coefficients.argtypes = [vp, vp, vp, vp]
    l.dfr_track_image.argtypes = [vp, i32, i32, vp, i32, i32, C.POINTER(Options), vp, vp, vp, i32]
    l.dfr_track_pyramid.argtypes = [vp, vp, vp, vp, vp, vp, i32, C.POINTER(Options), vp, vp, vp]
    return l


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def interpolate(m, r, c) -> np.float32:
    m = np.ascontiguousarray(m, dtype=np.float32)
    return np.float32(lib().dfr_interpolate(_p(m), m.shape[0], m.shape[1], float(r), float(c)))


def median9(values) -> np.float32:
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(9)
    return np.float32(lib().dfr_median9(_p(v)))


def gaussian(half_patch: int, k=(0.0, 0.0, 0.0)):
    """(ok, weights[(2h+1), (2h+1)], k = [k2, k4, k22]); k is the object's previous value, kept for half_patch 0."""
    size = max(2 * half_patch + 1, 1)
    w = np.zeros((size, size), np.float32)
    kk = np.array(k, dtype=np.float32)
    ok = lib().dfr_gaussian(int(half_patch), _p(w), _p(kk))
    return bool(ok), w, kk


def moments(image, half_patch: int, weights):
    """Six moment planes {S0, Sr, Sc, Src, Srr, Scc} of a uint8 or float32 image."""
    w = np.ascontiguousarray(weights, dtype=np.float32)
    img = np.asarray(image)
    out = np.zeros((6,) + img.shape, np.float32)
    if img.dtype == np.uint8:
        img = np.ascontiguousarray(img)
        lib().dfr_moments_u8(_p(img), img.shape[0], img.shape[1], int(half_patch), _p(w), _p(out))
    else:
        img = np.ascontiguousarray(img, dtype=np.float32)
        lib().dfr_moments_f32(_p(img), img.shape[0], img.shape[1], int(half_patch), _p(w), _p(out))
    return out


def coefficients(m6, k):
    """ConstructConstrainFunctionForPixel on six moments: (A 2x2, b 2)."""
    m = np.ascontiguousarray(m6, dtype=np.float32).reshape(6)
    kk = np.ascontiguousarray(k, dtype=np.float32).reshape(3)
    A = np.zeros(3, np.float32)
    b = np.zeros(2, np.float32)
    lib().dfr_coefficients(_p(m), _p(kk), _p(A), _p(b))
    return np.array([[A[0], A[1]], [A[1], A[2]]], np.float32), b


def track_image(ref, cur, opt: Options, k=(0.0, 0.0, 0.0), flow_r=None, flow_c=None):
    """Track(GrayImage, GrayImage, flow_rc): returns (ok, flow_r, flow_c, k).  A plane passed with ref's shape is the initial
    guess; any other plane (None included) is reset to zero, each independently."""
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    cur = np.ascontiguousarray(cur, dtype=np.uint8)
    valid = 0
    planes = []
    for bit, f in ((1, flow_r), (2, flow_c)):
        if f is not None and np.shape(f) == ref.shape:
            valid |= bit
            planes.append(np.array(f, dtype=np.float32, copy=True, order="C"))
        else:
            planes.append(np.zeros(ref.shape, np.float32))
    kk = np.array(k, dtype=np.float32)
    ok = lib().dfr_track_image(_p(ref), ref.shape[0], ref.shape[1], _p(cur), cur.shape[0], cur.shape[1], C.byref(opt), _p(kk), _p(planes[0]),
                               _p(planes[1]), valid)
    if not ok:
        return False, flow_r, flow_c, kk
    return True, planes[0], planes[1], kk


def track_pyramid(ref_levels, cur_levels, opt: Options, k=(0.0, 0.0, 0.0)):
    """Track(ImagePyramid, ImagePyramid, flow_rc): returns (ok, flow_r, flow_c, k) at level 0's size."""
    if len(ref_levels) != len(cur_levels) or len(ref_levels) == 0:
        return False, None, None, np.array(k, np.float32)
    n = len(ref_levels)
    refs = [np.ascontiguousarray(x, dtype=np.uint8) for x in ref_levels]
    curs = [np.ascontiguousarray(x, dtype=np.uint8) for x in cur_levels]
    rp = (C.c_void_p * n)(*[x.ctypes.data for x in refs])
    cp = (C.c_void_p * n)(*[x.ctypes.data for x in curs])
    rr = np.array([x.shape[0] for x in refs], np.int32)
    rc = np.array([x.shape[1] for x in refs], np.int32)
    cr = np.array([x.shape[0] for x in curs], np.int32)
    cc = np.array([x.shape[1] for x in curs], np.int32)
    fr = np.zeros(refs[0].shape, np.float32)
    fc = np.zeros(refs[0].shape, np.float32)
    kk = np.array(k, dtype=np.float32)
    ok = lib().dfr_track_pyramid(C.cast(rp, C.c_void_p), _p(rr), _p(rc), C.cast(cp, C.c_void_p), _p(cr), _p(cc), n, C.byref(opt), _p(kk), _p(fr), _p(fc))
    return bool(ok), fr, fc, kk


def same(a, b) -> bool:
    """Bit-identical float arrays, except that any NaN equals any NaN (the median)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
