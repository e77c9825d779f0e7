"""Plain numpy restatement of ImagePyramid::CreateImagePyramid, written from its definition alone (no code shared with
synth.build_pyramid or the oracle): level 0 is the image; level l + 1 is the truncating 2 x 2 box mean of level l's BYTES
(a mean of truncated means, not a mean over the 4^l source pixels), and sizes are floor-halved, so an odd trailing row or
column of a level contributes to nothing below it.

TEST INFRASTRUCTURE ONLY.
"""
import numpy as np


def halve(level: np.ndarray) -> np.ndarray:
    """One level step: out[r, c] = (p[2r, 2c] + p[2r, 2c + 1] + p[2r + 1, 2c] + p[2r + 1, 2c + 1]) // 4 on the bytes of `level`."""
    rows, cols = level.shape[0] // 2, level.shape[1] // 2
    p = level[: 2 * rows, : 2 * cols].astype(np.uint16)  # four bytes sum to at most 1020
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    return (s // 4).astype(np.uint8)


def max_levels(rows: int, cols: int) -> int:
    """The deepest pyramid of a rows x cols image whose last level still has a pixel."""
    n = 1
    while (rows >> n) > 0 and (cols >> n) > 0:
        n += 1
    return n


def pyramid(image: np.ndarray, levels: int):
    """[level 0 (a copy of the image), level 1, ..., level `levels` - 1]; refuses a level that would be empty."""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 2:
        raise ValueError("a 2-D uint8 image is expected")
    if not 1 <= levels <= max_levels(*image.shape):
        raise ValueError(f"{levels} levels do not fit a {image.shape[0]} x {image.shape[1]} image")
    out = [image.copy()]
    for _ in range(1, levels):
        out.append(halve(out[-1]))
    return out
