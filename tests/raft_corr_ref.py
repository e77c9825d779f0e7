"""ctypes binding of tests/raft_corr_ref.c — the scalar CPU restatement of RAFT's CorrelationPyramid.

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

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "raft_corr_ref.c")


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("raft_corr_ref", [_SRC], flags=STRICT + FMA)  # -mfma where the CPU has it: fmaf as one instruction (see above)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    l.rcr_row.argtypes = [vp, vp, i32, i32, i32, i32, i64, vp]
    l.rcr_row.restype = None
    l.rcr_pool.argtypes = [vp, i64, i32, i32, vp]
    l.rcr_pool.restype = None
    l.rcr_build.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    l.rcr_build.restype = i32
    l.rcr_sample.argtypes = [vp, i32, i32, i32, f32, f32, i32, i32]
    l.rcr_sample.restype = f32
    l.rcr_lookup.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp]
    l.rcr_lookup.restype = i32
    return l


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def layout(H: int, W: int, levels: int):
    """[(H_l, W_l)] per level, None when a level would be empty."""
    dims, h, w = [], H, W
    for _ in range(levels):
        if h == 0 or w == 0:
            return None
        dims.append((h, w))
        h, w = h // 2, w // 2
    return dims


def build(f0, f1, levels: int):
    """f0, f1: float32 [B, C, H, W].  Returns the list of levels, level l as [B*H*W, H_l, W_l]."""
    f0 = np.ascontiguousarray(f0, dtype=np.float32)
    f1 = np.ascontiguousarray(f1, dtype=np.float32)
    B, Cc, H, W = f0.shape
    dims = layout(H, W, levels)
    if dims is None:
        raise ValueError("a level would be empty")
    n = B * H * W
    vol = np.empty(sum(n * h * w for h, w in dims), np.float32)
    rc = lib().rcr_build(_p(f0), _p(f1), B, Cc, H, W, levels, _p(vol))
    assert rc == 0
    out, off = [], 0
    for h, w in dims:
        out.append(vol[off:off + n * h * w].reshape(n, h, w))
        off += n * h * w
    return out


def row(f0, f1, b: int, p: int):
    """Level-0 row (b, p) as [H, W]."""
    f0 = np.ascontiguousarray(f0, dtype=np.float32)
    f1 = np.ascontiguousarray(f1, dtype=np.float32)
    B, Cc, H, W = f0.shape
    out = np.empty((H, W), np.float32)
    lib().rcr_row(_p(f0), _p(f1), Cc, H, W, int(b), int(p), _p(out))
    return out


def pool(level):
    """2x2 pool of [n, h, w] slabs (floor halves)."""
    level = np.ascontiguousarray(level, dtype=np.float32)
    n, h, w = level.shape
    out = np.empty((n, h // 2, w // 2), np.float32)
    lib().rcr_pool(_p(level), n, h, w, _p(out))
    return out


def sample(slab, level: int, x: float, y: float, di: int, dj: int) -> np.float32:
    slab = np.ascontiguousarray(slab, dtype=np.float32)
    return np.float32(lib().rcr_sample(_p(slab), slab.shape[0], slab.shape[1], int(level), float(x), float(y), int(di), int(dj)))


def lookup(levels_list, coords, radius: int):
    """levels_list as build() returns; coords float32 [B, 2, H, W].  Returns [B, L*K, H, W]."""
    coords = np.ascontiguousarray(coords, dtype=np.float32)
    B, _, H, W = coords.shape
    L = len(levels_list)
    vol = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in levels_list]))
    K = (2 * radius + 1) ** 2
    out = np.empty((B, L * K, H, W), np.float32)
    rc = lib().rcr_lookup(_p(vol), B, H, W, L, int(radius), _p(coords), _p(out))
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
