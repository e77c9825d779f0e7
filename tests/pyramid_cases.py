"""Images and case tables shared by tests/test_pyramid_gpu.py (device pyramids == tests/pyramid_ref.py) and
tests/test_pyramid_ref_cpu.py (oracle.create_pyramid == tests/pyramid_ref.py on the very same tuples).

A case is (w, h, levels); the image is h rows by w columns.  The sizes are the smallest that reach each branch of
pyramid_kernels.hip; which branch a table is there for is said next to it and, per launch form, in the GPU test's docstrings.

TEST INFRASTRUCTURE ONLY.
"""
import functools

import numpy as np

from tests import pyramid_ref

MAX_LEVELS = 12  # FTK_MAX_LEVELS (include/ftk.h)

KINDS = ("noise", "coded", "extremes")  # the pyramid tests run all three

# The Harris tests add two kinds that reach the ends of the Sobel range: the three above do not (max |g| is 510 on extremes — a
# period-1 checkerboard has p[c + 1] == p[c - 1], so Sobel is 0 all over it and only the seam with the 255 half has a gradient —
# and about 870 on noise; their largest 5 x 5 sums are 2.6e6 and about 5.5e6, far below 2^24).
HARRIS_KINDS = ("extremes", "noise", "stripes", "jitter")
HARRIS_SIZES = [(97, 61), (300, 45)]  # (w, h): the existing small odd size; more than one 256-column block with a partial one


@functools.lru_cache(maxsize=None)
def image(kind: str, rows: int, cols: int) -> np.ndarray:
    """A seeded pure function of (rows, cols); the array is shared between tests and read-only.
      noise:    uniform random bytes
      coded:    (131 r + 17 c) & 255 — every pixel differs from all of its neighbours, so a swapped or shifted row / column
                shows in every output it touches
      extremes: 0 / 255 in a period-1 checkerboard on the left half, all 255 on the right half — 2 x 2 sums of 510 and 1020
      stripes:  0, 0, 255, 255, ... in vertical stripes on the upper half of the rows and horizontal ones on the lower half: Sobel
                is +-1020 in x (upper) or y (lower) on every pixel, and the 5 x 5 sums of squares are 25 * 1020^2 = 26 010 000
      jitter:   stripes with noise in the two low bits (0..3 and 252..255): |g| from 996 to 1020 and ODD products, so the sums
                pass 2^24 through values that fp32 cannot hold — a float accumulation rounds where the integer one does not"""
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    if kind == "noise":
        img = np.random.default_rng([20240601, rows, cols]).integers(0, 256, size=(rows, cols), dtype=np.uint8)
    elif kind == "coded":
        img = ((131 * r + 17 * c) & 255).astype(np.uint8)
    elif kind == "extremes":
        img = np.where(np.broadcast_to(c < cols // 2, (rows, cols)), 255 * ((r + c) & 1), 255).astype(np.uint8)
    elif kind in ("stripes", "jitter"):
        img = np.where(np.broadcast_to(r < rows // 2, (rows, cols)), 255 * ((c >> 1) & 1), 255 * ((r >> 1) & 1)).astype(np.uint8)
        if kind == "jitter":
            img ^= np.random.default_rng([20240602, rows, cols]).integers(0, 4, size=(rows, cols), dtype=np.uint8)
    else:
        raise KeyError(kind)
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _deepest_reference(kind: str, rows: int, cols: int):
    levels = pyramid_ref.pyramid(image(kind, rows, cols), min(MAX_LEVELS, pyramid_ref.max_levels(rows, cols)))
    for level in levels:
        level.setflags(write=False)
    return tuple(levels)


def reference(kind: str, rows: int, cols: int, levels: int):
    """tests/pyramid_ref.py's pyramid of image(kind, rows, cols): computed once per image, shared, read-only.  (A pyramid of n
    levels is the first n levels of any deeper one.)"""
    deepest = _deepest_reference(kind, rows, cols)
    assert 1 <= levels <= len(deepest)
    return deepest[:levels]


def _deepest(w: int, h: int, cap: int) -> int:
    return min(cap, pyramid_ref.max_levels(h, w))


def _unique(cases):
    out = []
    for case in cases:
        if case not in out:
            out.append(case)
    return out


def _checker(widths, heights):
    """Every other cell of the cross: each width at least twice, each height at least four times."""
    return [(w, h) for i, w in enumerate(widths) for j, h in enumerate(heights) if (i + j) % 2 == 0]


# --- wide tile: pyramid_fused_kernel<256, 16>, a host or pinned source with <= 5 levels -----------------------------------------
# widths: below / on / above one 16-byte segment (15, 16, 17) and one 256-column tile (255, 256, 257), a tile plus a partial
# segment either side of a segment edge (271, 273), two tiles (511, 513); heights: around one and two 16-row tiles.  At 5 levels a
# 16-row tile ends in ONE row of level 4.
WIDE_WIDTHS = (15, 16, 17, 255, 256, 257, 271, 273, 511, 513)
WIDE_HEIGHTS = (15, 16, 17, 31, 33)
WIDE = [(w, h, _deepest(w, h, 5)) for w in WIDE_WIDTHS for h in WIDE_HEIGHTS] + [(2, 2, 2)]  # (16 x 16 x 5, last level 1 x 1, is in the cross)
WIDE_TRIMMED = _unique([(w, h, _deepest(w, h, 5)) for w, h in _checker(WIDE_WIDTHS, WIDE_HEIGHTS)] + [(16, 16, 5), (2, 2, 2)])

# --- square tile: pyramid_fused_kernel<64, 64>, a device source at any depth, a host or pinned source at 6 and 7 levels ---------
# widths / heights around one, two and three 64-pixel tiles and around a segment edge behind a tile (79, 81); 2 levels (packed
# stores only), 6 and 7 (level widths of 2 and 1 per tile: the byte stores).  70 -> 35 -> 17 -> 8 and 90 -> 45 -> 22 -> 11 -> 5 have
# odd level widths, where the packed store's alignment changes row by row.
SQUARE_WIDTHS = (63, 64, 65, 79, 81, 127, 129, 191)
SQUARE_HEIGHTS = (63, 64, 65, 129)
SQUARE = [(w, h, n) for w, h in _checker(SQUARE_WIDTHS, SQUARE_HEIGHTS) for n in (2, 6, 7) if n <= pyramid_ref.max_levels(h, w)]
SQUARE = _unique(SQUARE + [(128, 128, 7), (64, 64, 7), (70, 70, 6), (90, 67, 6)])  # (the first two end in a 1 x 1 level)

# --- per-level kernel: downsample_kernel builds levels >= 7 from the level before ------------------------------------------------
DEEP = [
    (512, 128, 8),     # level 6 is 8 wide: level 7 (4 x 1) from the vector branch
    (576, 130, 8),     # level 6 is 9 wide: level 7 (4 x 1) is a full group of four on misaligned rows — the scalar loop
    (1024, 256, 9),    # 16 -> 8 -> 4: the vector branch on two levels, two groups per row on the first
    (1000, 300, 9),    # 15 -> 7 -> 3: scalar groups of 4 and 3, then of 3
    (2049, 2050, 12),  # every level up to FTK_MAX_LEVELS: 32 -> 16 -> 8 -> 4 vectorised, 4 -> 2 -> 1 scalar; last level 1 x 1
]

ONE_LEVEL = [(37, 29, 1)]  # a plain copy, no launch

# sources that start 1 and 3 bytes into their allocation: both tile forms, partial segments, odd level widths
MISALIGNED = [(17, 17, 5), (257, 33, 5), (273, 31, 5), (65, 65, 7), (129, 63, 6), (70, 70, 6)]
MISALIGNED_OFFSETS = (1, 3)

# launch form -> its cases (tests/test_pyramid_gpu.py has one test id per (form, case))
FORMS = {
    "build_host": ONE_LEVEL + WIDE + SQUARE + DEEP,
    "build_device": ONE_LEVEL + WIDE_TRIMMED + SQUARE + DEEP,
    "update_host": WIDE_TRIMMED + SQUARE,
    "update_device": WIDE_TRIMMED + SQUARE,
    "update_pinned": WIDE_TRIMMED + SQUARE,
    "update_pageable": WIDE_TRIMMED + SQUARE,
    "misaligned": MISALIGNED,
}


def all_cases():
    """Every (w, h, levels) any launch form uses, once."""
    return _unique([case for cases in FORMS.values() for case in cases])


def case_id(case) -> str:
    return "%dx%dx%d" % case
