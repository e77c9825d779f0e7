"""Shared synthetic scenes for the parity tests (small enough for the CPU oracle to finish in seconds)."""
from __future__ import annotations

import functools

import numpy as np

from feature_tracker_amd import synth


@functools.lru_cache(maxsize=None)
def scene(width, height, levels, motion="easy", kind="translation"):
    """Returns (ref_levels, cur_levels) host pyramids."""
    t = (3.3, -2.1) if motion == "easy" else (11.7, -8.4)
    if kind == "translation":
        ref, cur = synth.make_image_pair(width, height, t)
    elif kind == "similarity":
        ref, cur = synth.make_image_pair(width, height, t, rotation_deg=1.5, scale=1.02)
    elif kind == "flat":
        ref = np.full((height, width), 117, dtype=np.uint8)
        cur = ref.copy()
    else:
        raise ValueError(kind)
    return tuple(synth.build_pyramid(ref, levels)), tuple(synth.build_pyramid(cur, levels))


def features(n, width, height, half, seed=12345, border_fraction=0.05):
    return synth.make_features(n, width, height, seed=seed, margin=min(40.0, width / 8.0), border_fraction=border_fraction, half=half)


# ---- the throughput (tree) reduction mode: integer-exact scenes and the rounding-regime criterion --------------------------

def integer_scene(width, height, lo, hi, shift=(2, -1), seed=7, flat=None):
    """Low-contrast integer images (values in [lo, hi]) for one-level pyramids; cur is ref moved by the integer `shift` (u, v), and
    `flat` = (col0, row0, col1, row1) is one constant block in both.  Sampled at integer positions every bilinear weight is 0 or
    1, so every normal-equation factor is an integer and the sums are exact in any order while they stay below 2^24
    (integer_sum_bound)."""
    rs = np.random.RandomState(seed)
    base = rs.randint(lo, hi + 1, size=(height + 16, width + 16)).astype(np.uint8)
    ref = np.ascontiguousarray(base[8:8 + height, 8:8 + width])
    du, dv = shift
    cur = np.ascontiguousarray(base[8 - dv:8 - dv + height, 8 - du:8 - du + width])
    if flat is not None:
        c0, r0, c1, r1 = flat
        ref[r0:r1, c0:c1] = (lo + hi) // 2
        cur[r0:r1, c0:c1] = (lo + hi) // 2
    return ref, cur


def integer_features(n, width, height, half, seed=3, flat=None):
    """Integer positions: interior ones, the image's corners and edges, outside ones and (with `flat`) some in the flat block."""
    rs = np.random.RandomState(seed)
    fixed = [[0, 0], [width - 1, height - 1], [0, height - 1], [width - 1, 0], [1, height // 2], [width // 2, 1], [width - 2, height - 2],
             [-3, height // 3], [width + 2, 4], [5, -2], [-1, -1], [width, height]]
    if flat is not None:
        c0, r0, c1, r1 = flat
        fixed += [[(c0 + c1) // 2, (r0 + r1) // 2], [c0 + half + 1, r0 + half + 1]]
    inner = np.stack([rs.randint(0, width, max(n - len(fixed), 0)), rs.randint(0, height, max(n - len(fixed), 0))], axis=1)
    return np.concatenate([np.float32(fixed), inner.astype(np.float32)], axis=0)[:n].copy()


def integer_sum_bound(model, ref, cur, half_rows, half_cols):
    """An upper bound on sum |term| of every normal-equation sum of one feature, in int64: patch pixels x the largest term.  Basic
    terms are fx^2, fx fy, fy^2, fx ft, fy ft; affine ones carry x, y, xx, xy, yy (absolute coordinates) on top."""
    imgs = [np.asarray(ref, np.int64), np.asarray(cur, np.int64)]
    g = max(max(np.abs(i[:, 2:] - i[:, :-2]).max(), np.abs(i[2:, :] - i[:-2, :]).max()) for i in imgs)
    t = max(i.max() for i in imgs) - min(i.min() for i in imgs)
    patch = (2 * half_rows + 1) * (2 * half_cols + 1)
    term = g * max(g, t)
    if model == "affine":
        c = max(ref.shape) + max(half_rows, half_cols) + 1
        term *= c * c
    return int(patch * term)


def ulp(x):
    return float(np.spacing(np.float32(np.abs(np.asarray(x, np.float64)).max())))


def rounding_regime(tree, exact, wide, what=""):
    """The acceptance criterion of the tree mode against the wide-sum oracle: per feature e = |uv - uv_wide|_inf, then
    max e_tree <= 4 max e_exact + 2 ulp and median e_tree <= median e_exact + ulp (ulp of the largest |uv|).  Returns
    (ok, message, ratio of the error to the bound it has to meet); finite rows of `wide` only."""
    tree, exact, wide = (np.asarray(a, np.float64).reshape(len(wide), -1) for a in (tree, exact, wide))
    fin = np.isfinite(wide).all(axis=1)
    e_tree = np.abs(tree[fin] - wide[fin]).max(axis=1) if fin.any() else np.zeros(1)
    e_exact = np.abs(exact[fin] - wide[fin]).max(axis=1) if fin.any() else np.zeros(1)
    u = ulp(wide[fin]) if fin.any() else 0.0
    max_ok = e_tree.max() <= 4.0 * e_exact.max() + 2.0 * u
    med_ok = np.median(e_tree) <= np.median(e_exact) + u
    # how far past the criterion: the larger of the two ratios (features with near-singular normal equations can make both
    # maxima large; the median then carries the verdict)
    ratio = max(e_tree.max() / (4.0 * e_exact.max() + 2.0 * u), np.median(e_tree) / (np.median(e_exact) + u))
    msg = (f"{what}: max e_tree {e_tree.max():.3g} vs max e_exact {e_exact.max():.3g}, median {np.median(e_tree):.3g} vs "
           f"{np.median(e_exact):.3g}, ulp {u:.3g} ({fin.sum()} rows)")
    return bool(max_ok and med_ok), msg, float(ratio)
