"""ctypes binding of tests/keypoint_decode_ref.c — the scalar CPU restatement of the keypoint decoder — with the inputs the
CPU and GPU tests share and an independent numpy float64 composition of the same five steps.

TEST INFRASTRUCTURE ONLY: compiled on first use (gcc -O3 -ffp-contract=off) into a temporary directory; nothing under
feature_tracker_amd/ may import it, and it imports nothing from there.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests.ref_build import compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "keypoint_decode_ref.c")

CONTRACT = 0
MUTANTS = {"dustbin_left_out_of_the_denominator": 1, "k_div_8_and_k_mod_8_exchanged": 2, "no_cell_centre_shift": 3, "higher_pixel_index_first_on_a_tie": 4,
           "normalised_per_corner_before_blending": 5}
LAYOUTS = ("chw", "hwc")


@functools.lru_cache(maxsize=None)
def lib():
    l = compile_ref("keypoint_decode_ref", [_SRC])
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    l.kdr_decode.argtypes = [vp, i32, i32, vp, i32, i64, i64, i64, i32, C.c_float, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    l.kdr_decode.restype = i32
    return l


class Result:
    """What one call leaves: uv [K, 2], scores [K], descriptors [K, D], count (int), heatmap [H, W], survivors (S, int)."""


OUTPUTS = ("uv", "scores", "descriptors", "heatmap")


def decode(semi, desc, max_keypoints=300, min_score=0.1, min_distance=20, border=4, occupied=None, occupied_mask=None, layout="chw", variant=CONTRACT) -> Result:
    """``desc`` is [D, Hc, Wc]; ``layout`` "hwc" hands the restatement a channel-last copy with its strides."""
    semi = np.ascontiguousarray(semi, np.float32)
    assert semi.ndim == 3 and semi.shape[0] == 65
    hc, wc = semi.shape[1:]
    desc = np.asarray(desc, np.float32)
    d = desc.shape[0]
    assert desc.shape == (d, hc, wc)
    if layout == "chw":
        mem, strides = np.ascontiguousarray(desc), (hc * wc, wc, 1)
    else:
        mem, strides = np.ascontiguousarray(desc.transpose(1, 2, 0)), (1, wc * d, d)
    K = int(max_keypoints)
    r = Result()
    r.uv, r.scores, r.descriptors = np.full((K, 2), -1, np.float32), np.full(K, -1, np.float32), np.full((K, d), -1, np.float32)
    r.heatmap = np.full((8 * hc, 8 * wc), -1, np.float32)
    count, survivors = np.zeros(1, np.int32), np.zeros(1, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    occ = None if occupied is None else np.ascontiguousarray(occupied, np.float32).reshape(-1, 2)
    flags = None if occupied_mask is None else np.ascontiguousarray(occupied_mask, np.uint8)
    rc = lib().kdr_decode(p(semi), hc, wc, p(mem), d, strides[0], strides[1], strides[2], K, float(min_score), int(min_distance), int(border), p(occ),
                          p(flags), 0 if occ is None else len(occ), int(variant), p(r.uv), p(r.scores), p(r.descriptors), p(count), p(r.heatmap), p(survivors))
    assert rc == 0
    r.count, r.survivors = int(count[0]), int(survivors[0])
    return r


def same(a, b) -> bool:
    """Bit for bit, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def same_results(a, b) -> list:
    """The names of the outputs in which two results differ by a bit."""
    bad = [name for name in OUTPUTS if not same(getattr(a, name), getattr(b, name))]
    return bad + (["count"] if a.count != b.count else [])


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def heads(hc, wc, d, seed):
    """Seeded random heads: logits N(0, 2.5^2) (a cell's strongest pixel scores 0.1 .. 0.6), descriptors N(0, 1)."""
    rng = np.random.default_rng(seed)
    return _frozen((2.5 * rng.standard_normal((65, hc, wc))).astype(np.float32), rng.standard_normal((d, hc, wc)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def occupied_points(hc, wc, n, seed):
    """n points over the image and a little beyond it, and a mask that drops every third."""
    rng = np.random.default_rng(seed)
    uv = rng.uniform([-3.0, -3.0], [8 * wc + 3.0, 8 * hc + 3.0], (n, 2)).astype(np.float32)
    return _frozen(uv, (np.arange(n) % 3 != 0).astype(np.uint8))


# name -> (hc, wc, d, seed, min_score, min_distance, border, n_occupied (0: none), with_mask): the shapes of the GPU tests.  The grids cover
# one cell, a partial wave, a full wave plus one cell in a row, and several tile rows.
CASES = {
    "one_cell": (1, 1, 64, 11, 0.02, 1, 0, 0, False),
    "partial_wave_d4": (3, 5, 65, 12, 0.05, 4, 4, 0, False),
    "partial_wave_d1": (3, 5, 256, 13, 0.1, 1, 0, 0, False),
    "wave_plus_one_d9": (2, 65, 256, 14, 0.05, 9, 0, 0, False),
    "wave_plus_one_d4": (2, 65, 1, 15, 0.05, 4, 4, 0, False),
    "tile_rows_d4_occupied": (9, 17, 64, 16, 0.05, 4, 4, 40, False),
    "tile_rows_d9_masked": (9, 17, 65, 17, 0.05, 9, 4, 40, True),
    "tile_rows_d1": (9, 17, 1, 18, 0.2, 1, 0, 0, False),
}


def case(name):
    """name -> (semi, desc, kwargs of decode without max_keypoints)."""
    hc, wc, d, seed, min_score, min_distance, border, n_occ, with_mask = CASES[name]
    semi, desc = heads(hc, wc, d, seed)
    kw = dict(min_score=min_score, min_distance=min_distance, border=border)
    if n_occ:
        uv, mask = occupied_points(hc, wc, n_occ, seed + 100)
        kw.update(occupied=uv, occupied_mask=mask if with_mask else None)
    return semi, desc, kw


def with_peak(semi, cy, cx, k, height=12.0):
    """A writable copy of the logits with pixel k of cell (cy, cx) raised to ``height``."""
    out = np.array(semi, np.float32, copy=True)
    out[k, cy, cx] = height
    return out


def tie_heads():
    """Two equal cells in one window (adjacent cells: the same pixel of either lies 8 apart, inside min_distance 9) and a third far away."""
    semi, desc = heads(3, 5, 64, 21)
    semi = with_peak(semi, 0, 0, 27, 9.0)  # strong enough that no neighbour suppresses it
    semi[:, 0, 1] = semi[:, 0, 0]
    semi[:, 2, 4] = semi[:, 0, 0]
    return semi, desc


def corner_heads():
    """A keypoint in each image corner (border 0): the clamps of the descriptor sample."""
    semi, desc = heads(3, 5, 65, 22)
    for cy, cx, k in ((0, 0, 0), (0, 4, 7), (2, 0, 56), (2, 4, 63)):
        semi = with_peak(semi, cy, cx, k)
    return semi, desc


def hostile_heads():
    """NaN, +-inf, +-1e30 logits, a cell of all -inf, and descriptors with NaN, inf, 1e30 and values whose squares are subnormal."""
    semi, desc = heads(3, 5, 65, 23)
    semi, desc = np.array(semi, copy=True), np.array(desc, copy=True)
    semi[5, 0, 0] = np.nan
    semi[0, 0, 1] = np.nan          # x_0 = NaN: m = NaN
    semi[9, 0, 2] = np.inf
    semi[3, 0, 3] = -np.inf
    semi[7, 0, 4] = 1e30
    semi[8, 1, 0] = -1e30
    semi[:, 1, 1] = -np.inf
    semi[64, 1, 2] = 1e30           # the dustbin takes everything: every score of the cell is +0
    semi[:, 1, 3] = 1e30
    desc[3, 2, 0] = np.nan
    desc[4, 2, 1] = np.inf
    desc[5, 2, 2] = -np.inf
    desc[:, 2, 3] = 1e30
    desc[:, 2, 4] *= 1e-21
    desc[:, 1, 4] = 0.0
    return semi, desc


# ---- the float64 composition ---------------------------------------------------------------------------------------------------------

def decode_float64(semi, desc, max_keypoints, min_score, min_distance, border, occupied=None, occupied_mask=None):
    """softmax, shuffle, the same selection rule on float64 scores, sampling, normalise, all in numpy float64: (pixels [n] (flat indices,
    strongest first), heatmap [H, W], descriptor_of(pixel) -> [D])."""
    x = np.asarray(semi, np.float64)
    hc, wc = x.shape[1:]
    H, W = 8 * hc, 8 * wc
    e = np.exp(x - x.max(axis=0, keepdims=True))
    prob = e / e.sum(axis=0, keepdims=True)
    heat = prob[:64].reshape(8, 8, hc, wc).transpose(2, 0, 3, 1).reshape(H, W)
    inside = np.zeros((H, W), bool)
    inside[border:H - border, border:W - border] = True
    cand = (heat > min_score) & inside
    d = max(int(min_distance), 1)
    reach = d - 1
    if occupied is not None:
        for i, (u, v) in enumerate(np.asarray(occupied, np.float64)):
            if occupied_mask is not None and not occupied_mask[i]:
                continue
            cx, cy = int(np.clip(np.floor(u + 0.5), 0, W - 1)), int(np.clip(np.floor(v + 0.5), 0, H - 1))
            cand[max(cy - reach, 0):cy + reach + 1, max(cx - reach, 0):cx + reach + 1] = False
    masked = np.where(cand, heat, -np.inf)
    survivors = []
    for y, xx in zip(*np.nonzero(cand)):
        win = masked[max(y - reach, 0):y + reach + 1, max(xx - reach, 0):xx + reach + 1]
        s = masked[y, xx]
        if s < win.max():
            continue
        ys, xs = np.nonzero(win == s)  # equal scores: the lower pixel index
        first = (ys[0] + max(y - reach, 0)) * W + xs[0] + max(xx - reach, 0)
        if first == y * W + xx:
            survivors.append((-s, y * W + xx))
    survivors.sort()
    pixels = np.array([i for _, i in survivors[:max_keypoints]], np.int64)
    dd = np.asarray(desc, np.float64)

    def descriptor_of(pixel):
        px, py = pixel % W, pixel // W
        xc, yc = np.clip((px - 3.5) / 8.0, 0, wc - 1), np.clip((py - 3.5) / 8.0, 0, hc - 1)
        x0, y0 = int(xc), int(yc)
        x1, y1 = min(x0 + 1, wc - 1), min(y0 + 1, hc - 1)
        fx, fy = xc - x0, yc - y0
        v = (1 - fx) * (1 - fy) * dd[:, y0, x0] + fx * (1 - fy) * dd[:, y0, x1] + (1 - fx) * fy * dd[:, y1, x0] + fx * fy * dd[:, y1, x1]
        return v / max(np.linalg.norm(v), 1e-12)

    return pixels, heat, descriptor_of
