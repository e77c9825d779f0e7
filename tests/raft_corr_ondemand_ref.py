"""ctypes binding of tests/raft_corr_ondemand_ref.c — the scalar CPU restatement of RAFT's on-demand correlation.

TEST INFRASTRUCTURE ONLY: compiled on first use with tests/raft_corr_ref.py's flags (gcc -O3 -ffp-contract=off, plus -mfma where the CPU
has it) into a temporary directory; nothing under feature_tracker_amd/ may import it.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests.raft_corr_ref import layout, same  # noqa: F401  (same: bit-identical, any NaN equals any NaN)
from tests.ref_build import FMA, STRICT, compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "raft_corr_ondemand_ref.c")


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("raft_corr_ondemand_ref", [_SRC], flags=STRICT + FMA)  # -mfma where the CPU has it: fmaf as one instruction (see above)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    l.rco_pool.argtypes, l.rco_pool.restype = [vp, i64, i32, i32, vp], None
    l.rco_row.argtypes, l.rco_row.restype = [vp, vp, i32, i64, i64, i32, i64, vp], None
    l.rco_sample.argtypes, l.rco_sample.restype = [vp, i32, i32, i32, f32, f32, i32, i32], f32
    l.rco_floor_ix.argtypes, l.rco_floor_ix.restype = [i32, i32, vp, i64, i32, vp], None
    l.rco_lookup.argtypes, l.rco_lookup.restype = [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp], i32
    return l


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float32)


def pool(fmap):
    """2x2 pool of a feature map [B, C, h, w] (floor halves)."""
    fmap = _f32(fmap)
    B, Cc, h, w = fmap.shape
    out = np.empty((B, Cc, h // 2, w // 2), np.float32)
    lib().rco_pool(_p(fmap), B * Cc, h, w, _p(out))
    return out


def pooled_maps(fmap1, levels: int):
    """[fmap1, pool(fmap1), ...]: ``levels`` maps."""
    maps = [_f32(fmap1)]
    for _ in range(levels - 1):
        maps.append(pool(maps[-1]))
    return maps


def row(f0, f1_level, b: int, p: int):
    """The correlation of query pixel ``p`` of item ``b`` with every position of one (pooled) level of fmap1, as [h, w]."""
    f0, f1_level = _f32(f0), _f32(f1_level)
    B, Cc, H, W = f0.shape
    h, w = f1_level.shape[2:]
    out = np.empty((h, w), np.float32)
    lib().rco_row(_p(f0), _p(f1_level), Cc, H * W, h * w, int(b), int(p), _p(out))
    return out


def sample(slab, level: int, x: float, y: float, di: int, dj: int) -> np.float32:
    slab = _f32(slab)
    return np.float32(lib().rco_sample(_p(slab), slab.shape[0], slab.shape[1], int(level), float(x), float(y), int(di), int(dj)))


def floor_ix(w: int, level: int, xs, dj: int):
    """floor(ix) of the sampler for every coordinate of ``xs`` at window offset ``dj`` in a level of width ``w``."""
    xs = _f32(xs).ravel()
    out = np.empty_like(xs)
    lib().rco_floor_ix(int(w), int(level), _p(xs), xs.size, int(dj), _p(out))
    return out


def lookup(f0, f1, levels: int, coords, radius: int):
    """f0, f1 float32 [B, C, H, W]; coords [B, 2, H, W].  Returns [B, L*K, H, W]."""
    f0, f1, coords = _f32(f0), _f32(f1), _f32(coords)
    B, Cc, H, W = f0.shape
    assert f1.shape == f0.shape and coords.shape == (B, 2, H, W)
    if layout(H, W, levels) is None:
        raise ValueError("a level would be empty")
    K = (2 * radius + 1) ** 2
    out = np.empty((B, levels * K, H, W), np.float32)
    rc = lib().rco_lookup(_p(f0), _p(f1), B, Cc, H, W, int(levels), int(radius), _p(coords), _p(out))
    assert rc == 0
    return out
