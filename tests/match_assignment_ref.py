"""ctypes binding of tests/match_assignment_ref.c — the scalar CPU restatement of LightGlue's assignment head — with the
inputs the CPU and GPU tests share.

TEST INFRASTRUCTURE ONLY: compiled on first use (gcc -O3 -ffp-contract=off) into a temporary directory; nothing under
feature_tracker_amd/ may import it, and it imports nothing from there.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests.ref_build import compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "match_assignment_ref.c")

CONTRACT = 0
MUTANTS = {"column_softmax_left_out": 1, "scale_on_one_side_only": 2, "dustbin_from_ls_z": 3, "invalid_columns_in_a_rows_normaliser": 4,
           "z_from_the_projected_descriptor": 5}
SENTINEL = np.float32(-12345.0)  # what a strided output holds behind each row before the call, and must hold after it


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("match_assignment_ref", [_SRC])
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    l.mar_assign.argtypes = [vp, i32, vp, i32, i32, vp, vp, f32, vp, vp, i32, vp, C.c_int64]
    l.mar_assign.restype = i32
    for name in ("mar_exp_c", "mar_log_c", "mar_ls"):
        getattr(l, name).argtypes = [f32]
        getattr(l, name).restype = f32
    return l


def default_scale(dim: int) -> float:
    """Upstream's dim ** -0.25 per side, as the float32 the library receives."""
    return float(np.float32(dim ** -0.25))


def assign(desc0, desc1, weights=None, bias=None, scale=None, count0=None, count1=None, row_stride=None, variant=CONTRACT):
    """scores [M + 1, N + 1] float32 (a view of a strided buffer whose padding holds SENTINEL).  ``weights`` [D + 1, D] and ``bias``
    [D + 1] packed as the library takes them, or None."""
    desc0, desc1 = np.ascontiguousarray(desc0, np.float32), np.ascontiguousarray(desc1, np.float32)
    (m, d), n = desc0.shape, desc1.shape[0]
    assert desc1.shape == (n, d)
    if weights is not None:
        weights, bias = np.ascontiguousarray(weights, np.float32), np.ascontiguousarray(bias, np.float32)
        assert weights.shape == (d + 1, d) and bias.shape == (d + 1,)
    s = default_scale(d) if scale is None else float(np.float32(scale))
    stride = n + 1 if row_stride is None else int(row_stride)
    buf = np.full((m + 1, stride), SENTINEL, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    word = lambda c: None if c is None else p(np.array([c], np.int32))  # noqa: E731
    rc = lib().mar_assign(p(desc0), m, p(desc1), n, d, p(weights), p(bias), s, word(count0), word(count1),
                          int(variant), p(buf), stride)
    assert rc == 0
    return buf[:, :n + 1]


def log_c(x) -> np.ndarray:
    f = lib().mar_log_c
    return np.array([f(float(v)) for v in np.asarray(x, np.float32).ravel()], np.float32)


def ls(z: float) -> np.float32:
    return np.float32(lib().mar_ls(float(np.float32(z))))


def same(a, b) -> bool:
    """Bit for bit, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def pack(final_w, final_b, match_w, match_b):
    """Upstream's four tensors as the library takes them: [D + 1, D] and [D + 1]."""
    return (np.ascontiguousarray(np.concatenate([final_w, match_w.reshape(1, -1)], 0), np.float32),
            np.ascontiguousarray(np.concatenate([final_b, match_b.reshape(1)], 0), np.float32))


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def descriptors(m, n, d, seed):
    """For d >= 4 unit-length rows times 4 (so that a true pair's similarity stands out after the scale); the first min(m, n) rows of the second set
    are a permutation of the first set's, with noise."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((m, d))
    b = rng.standard_normal((n, d))
    k = min(m, n)
    perm = rng.permutation(k)
    b[perm] = a[:k] + 0.3 * rng.standard_normal((k, d))
    if d >= 4:  # (a unit vector of one to three entries has too few values to tell rows apart)
        a /= np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-9)
        b /= np.maximum(np.linalg.norm(b, axis=1, keepdims=True), 1e-9)
        a, b = 4.0 * a, 4.0 * b
    return _frozen(a.astype(np.float32), b.astype(np.float32))


@functools.lru_cache(maxsize=None)
def head_weights(d, seed):
    """final_proj [D, D] close to a rotation-free identity plus noise (pairs stay pairs), matchability [1, D], biases."""
    rng = np.random.default_rng(seed)
    fw = (np.eye(d) + rng.standard_normal((d, d)) / np.sqrt(d) * 0.5).astype(np.float32)
    fb = (0.1 * rng.standard_normal(d)).astype(np.float32)
    mw = (rng.standard_normal((1, d)) / np.sqrt(d)).astype(np.float32)
    mb = (0.5 * rng.standard_normal(1)).astype(np.float32)
    return _frozen(fw, fb, mw, mb)


# (M, N, D, seed): the shapes of the GPU tests.  M, N cover one lane, a partial 32-tile, a tile plus one, one full set of partials, a set
# plus one and several tiles; D covers 1, one k-step, an odd pad, whole vector chunks, a chunk plus one, and the usual 256.
SHAPES = ((1, 1, 1, 101), (1, 130, 64, 102), (31, 33, 2, 103), (33, 31, 3, 104), (64, 64, 64, 105), (65, 64, 65, 106), (64, 65, 256, 107),
          (130, 130, 256, 108), (130, 1, 3, 109), (31, 130, 65, 110), (65, 33, 1, 111), (33, 65, 2, 112))


def case(shape, with_weights):
    """(desc0, desc1, kwargs of assign): weights and bias packed, or the default scale."""
    m, n, d, seed = shape
    a, b = descriptors(m, n, d, seed)
    if not with_weights:
        return a, b, {}
    w, bias = pack(*head_weights(d, seed + 1000))
    return a, b, dict(weights=w, bias=bias)


def hostile(shape):
    """A writable copy of a case's descriptors with NaN, +-inf, +-1e30 and an all-equal row."""
    m, n, d, seed = shape
    a, b = (np.array(x, copy=True) for x in descriptors(m, n, d, seed))
    a[1, 0] = np.nan
    a[3, d - 1] = np.inf
    a[5, 0] = -np.inf
    a[7] = 1e30
    a[9] = -1e30
    a[11] = 0.25
    b[2, 0] = np.nan
    b[4] = 1e30
    b[6, d - 1] = -np.inf
    b[8] = 0.25
    return a, b
