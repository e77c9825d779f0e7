"""ctypes binding of tests/nn_match_ref.c — the scalar CPU restatement of NNFeatureMatcher::Match's post-processing.

TEST INFRASTRUCTURE ONLY: compiled on first use (gcc -O2 -fno-fast-math: the comparisons must keep their NaN behaviour) into a
temporary directory; nothing under feature_tracker_amd/ may import it.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests.ref_build import compile_ref

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nn_match_ref.c")

TRACKED, LARGE_RESIDUAL = 1, 2


@functools.lru_cache(maxsize=None)
def lib():
    # not STRICT: -O2, no -ffp-contract=off, no -lm; the source compares and copies floats and has no arithmetic on them to contract
    l = compile_ref("nn_match_ref", [_SRC], flags=["-O2", "-std=c99", "-fno-fast-math"], libs=())
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    l.nmr_scores.argtypes = [vp, i32, i32, i64, f32, vp, vp, vp, C.c_int]
    l.nmr_scores.restype = None
    l.nmr_list.argtypes = [vp, i32, i32, i32, vp, vp]
    l.nmr_list.restype = None
    l.nmr_fill.argtypes = [vp, i32, vp, i32, vp]
    l.nmr_fill.restype = None
    return l


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def match_scores(scores, min_score: float, mutant: bool = False):
    """scores: float32 [n_ref, n_cur] or [B, n_ref, n_cur] (any strides: copied).  Returns (match_index int32, status uint8) of the
    leading shape."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    batched = s.ndim == 3
    s3 = s if batched else s[None]
    B, n_ref, n_cur = s3.shape
    assert n_ref >= 1 and n_cur >= 1
    idx = np.empty((B, n_ref), np.int32)
    st = np.empty((B, n_ref), np.uint8)
    col = np.empty(n_cur, np.int32)
    for b in range(B):
        item = np.ascontiguousarray(s3[b])
        lib().nmr_scores(_p(item), n_ref, n_cur, n_cur, np.float32(min_score), _p(col), _p(idx[b]), _p(st[b]), int(mutant))
    return (idx, st) if batched else (idx[0], st[0])


def match_list(matches, n_ref: int, n_cur: int):
    m = np.ascontiguousarray(matches, dtype=np.int64).reshape(-1, 2)
    idx = np.empty(n_ref, np.int32)
    st = np.empty(n_ref, np.uint8)
    lib().nmr_list(_p(m), m.shape[0], n_ref, n_cur, _p(idx), _p(st))
    return idx, st


def fill(match_index, cur_uv):
    idx = np.ascontiguousarray(match_index, dtype=np.int32)
    uv = np.ascontiguousarray(cur_uv, dtype=np.float32).reshape(-1, 2)
    out = np.empty_like(uv)
    lib().nmr_fill(_p(idx), idx.shape[0], _p(uv), uv.shape[0], _p(out))
    return out


# ---- an independent pure-Python double loop (no shared code with the C file: Python floats compare as IEEE doubles, and every
# float32 is exactly a double, so the comparisons agree) ----

def match_scores_python(scores, min_score: float):
    s = np.asarray(scores, dtype=np.float32)
    n_ref, n_cur = s.shape
    rows = [[float(x) for x in r] for r in s]
    thr = float(np.float32(min_score))
    col_best = []
    for j in range(n_cur):
        b, m = 0, rows[0][j]
        for i in range(1, n_ref):
            if rows[i][j] > m:
                b, m = i, rows[i][j]
        col_best.append(b)
    idx, st = [], []
    for i in range(n_ref):
        b, m = 0, rows[i][0]
        for j in range(1, n_cur):
            if rows[i][j] > m:
                b, m = j, rows[i][j]
        ok = (not (m < thr)) and col_best[b] == i
        idx.append(b if ok else -1)
        st.append(TRACKED if ok else LARGE_RESIDUAL)
    return np.array(idx, np.int32), np.array(st, np.uint8)


# ---- shared case builders (CPU and GPU tests) ----

NAN, INF = np.float32("nan"), np.float32("inf")


def quantised(rng, shape, levels=8, nan_rate=0.0, specials=False):
    """Scores drawn from <= `levels` values so that most rows and columns tie; optionally with NaN / +-inf / +-0 mixed in."""
    values = np.float32([-7.5, -3.0, -2.999999, -0.0, 0.0, 1.25, -1e30, 3.5][:levels])
    if specials:
        values = np.float32([-INF, -3.0, -0.0, 0.0, INF, -5.0, NAN, 2.0][:levels])
    s = values[rng.integers(0, len(values), size=shape)]
    if nan_rate > 0:
        s = np.where(rng.random(shape) < nan_rate, NAN, s).astype(np.float32)
    return np.ascontiguousarray(s, dtype=np.float32)


def hand_cases():
    """(name, scores, min_score, expected match_index) — answers derived by hand from the contract, not from any code."""
    f = np.float32
    c = []
    c.append(("ties -> lowest index", f([[1, 1], [1, 1]]), -3.0, [0, -1]))          # col_best = [0, 0]; row 0 -> 0 mutual; row 1 -> 0, col 0 belongs to row 0
    c.append(("+-0 tie", f([[-0.0, 0.0], [0.0, -0.0]]), -3.0, [0, -1]))           # all four compare equal
    c.append(("-0 then +0 in a row", f([[-5, -0.0, 0.0]]), -3.0, [1]))            # +0 does not beat -0
    c.append(("NaN at row index 0", f([[NAN, 9], [1, 2]]), -3.0, [0, -1]))         # row 0 keeps j = 0 (NaN max passes the threshold); col 0: NaN at i = 0 keeps it; row 1 -> 1, col 1 -> row 0
    c.append(("NaN at i = 0 keeps its column, at j > 0 never wins", f([[1, NAN], [0, 2]]), -3.0, [0, -1]))  # col_best = [0, 0]; row 0 -> 0; row 1 -> 1, col 1 -> row 0
    c.append(("NaN among larger and smaller scores", f([[1, NAN, 3], [4, 5, NAN]]), -3.0, [2, -1]))        # col_best = [1, 0, 0]; row 0 -> 2 mutual; row 1 -> 1, col 1 -> row 0
    c.append(("NaN below index 0 in a column", f([[1, 0], [NAN, 2]]), -3.0, [0, -1]))  # col 0 -> 0 (NaN at i = 1 loses), col 1 -> 1; row 0 -> 0 ok; row 1: NaN at j = 0 keeps it -> 0, col 0 -> 0: unmatched
    c.append(("all -inf", f([[-INF, -INF], [-INF, -INF]]), -INF, [0, -1]))         # index 0 everywhere; -inf < -inf is false: passes
    c.append(("all -inf under a finite threshold", f([[-INF, -INF]]), -3.0, [-1]))
    c.append(("threshold equal to the maximum", f([[-3.0, -4.0]]), -3.0, [0]))     # -3 < -3 is false
    c.append(("threshold one ulp above", f([[-3.0, -4.0]]), np.nextafter(f(-3.0), f(0)), [-1]))
    c.append(("NaN threshold passes all", f([[-100.0, -200.0]]), NAN, [0]))
    c.append(("n_ref > n_cur", f([[5], [6], [6]]), -3.0, [-1, 0, -1]))              # col 0 -> first 6 = row 1
    c.append(("1 x 1", f([[0.5]]), -3.0, [0]))
    c.append(("1 x 1 below", f([[-3.5]]), -3.0, [-1]))
    c.append(("1 x M", f([[1, 7, 7, 2]]), -3.0, [1]))
    c.append(("N x 1", f([[1], [7], [7], [2]]), -3.0, [-1, 0, -1, -1]))
    c.append(("permutation", f([[0, 9, 0], [0, 0, 9], [9, 0, 0]]), -3.0, [1, 2, 0]))
    c.append(("not mutual", f([[5, 4], [6, 1]]), -3.0, [-1, 0]))                    # row 0 -> 0 but col 0 -> row 1; row 1 -> 0 mutual
    return c


def list_cases():
    """(name, matches, n_ref, n_cur, expected match_index)."""
    big = 1 << 31
    return [
        ("plain", [[0, 1], [2, 0]], 3, 3, [1, -1, 0]),
        ("duplicates: last wins", [[1, 0], [1, 2], [1, 1]], 3, 3, [-1, 1, -1]),
        ("negatives", [[-1, 0], [0, -1], [1, 1]], 2, 2, [-1, 1]),
        ("out of range", [[2, 0], [0, 2], [1, 0]], 2, 2, [-1, 0]),
        ("beyond 2^31", [[big, 0], [0, big + 1], [big + 1, big], [-big - 5, 0], [0, 1]], 2, 2, [1, -1]),
        ("int64 that truncates into range", [[(1 << 32) + 1, 0], [0, (1 << 32)]], 3, 3, [-1, -1, -1]),
        ("idx_ref bounded by n_cur", [[2, 0], [1, 0]], 4, 2, [-1, 0, -1, -1]),   # idx_ref 2 >= n_cur: not applied
        ("idx_ref bounded by n_ref", [[2, 0], [1, 3]], 2, 5, [-1, 3]),
        ("empty list", np.zeros((0, 2), np.int64), 3, 2, [-1, -1, -1]),
        ("n_cur 0", [[0, 0]], 2, 0, [-1, -1]),
        ("later invalid row does not undo", [[0, 1], [0, 7]], 2, 2, [1, -1]),
    ]
