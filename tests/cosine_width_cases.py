"""The widths and inputs of the cosine matcher's width tests (tests/test_cosine_widths_cpu.py, tests/test_cosine_widths_gpu.py): one
place that names them and builds them, deterministic and seeded by the width.  No fixtures, no device.

CosineMatcher accepts 1 <= dim <= 4096 (csrc/match_plan.h) and picks its contraction by dim_pad = align_up(dim, 64): the
register-stationary kernel with 4, 8, 12 or 16 K steps up to 256, the chunked pair with dim_pad / 64 chunks above; the exact side
(eigen_dot_octet) branches on dim % 8, dim < 4 and dim < 8.  WIDTHS walks all of that at one small shape with ragged tails in every
row group (130 x 200: two 128-row chunked tiles on both sides, four 64-row tiles of candidates, a quarter of a 512-row group)."""
import collections
import functools

import numpy as np

from feature_tracker_amd import synth

WIDTHS = tuple(range(1, 41)) + (63, 64, 65, 100, 127, 128, 129, 130, 136, 160, 191, 192, 193, 255, 256, 257, 264, 319, 320, 321, 511, 512, 513, 1000, 1021,
                                2048, 4095, 4096)
N_REF, N_CUR = 130, 200
WINDOW = (60, 45)               # NearbyMatch: kMaxValidPredictColDistance, kMaxValidPredictRowDistance
FORCE_THRESHOLDS = (0.1, 0.6)
NEARBY_THRESHOLD = 0.9
HEAVY_TAIL_MIN_DIM = 512
K_MARGIN = 1.5e-3               # kCosineMargin (csrc/ftk_device.h)
K_MARGIN_PER_K = 1.75e-7        # kCosineMarginPerK
IRREGULAR_CAP = 64              # kCosineIrregularCap
CAND_CAP = 64                   # kCosineCandCap

# the near-tie group: 40 reference rows on both sides of the 64-row (a wave's rows) and the 128-row (a chunked tile) boundaries, 30
# candidates in two runs that cross the 64- and the 128-candidate tile boundaries
TIE_ROWS = tuple(range(50, 86)) + (126, 127, 128, 129)
TIE_SLOTS = tuple(range(56, 72)) + tuple(range(121, 135))
DUP_LATER = (3, 180)    # (k, slot): candidate k of the group copied to a HIGHER index: the original must win
DUP_EARLIER = (7, 5)    # candidate k copied to a LOWER index: the copy must win

Case = collections.namedtuple("Case", "ref cur pred_uv cur_uv")


def dim_pad(dim):
    return -(-dim // 64) * 64


def plan_margin(dim):
    """CosinePlan::margin (csrc/match_plan.cpp), in double."""
    return K_MARGIN if dim_pad(dim) <= 256 else K_MARGIN + K_MARGIN_PER_K * (dim_pad(dim) - 256)


def eigen_dot_branches(dim):
    """The branches eigen_dot_octet (csrc/float_matcher_kernels.hip) and orc_eigen_dot take at this size:
    (aligned_size == 0, aligned_size == 4, aligned_size > aligned_end2, size > aligned_size)."""
    aligned_size, aligned_end2 = dim // 4 * 4, dim // 8 * 8
    return (aligned_size == 0, aligned_size == 4, aligned_size > aligned_end2, dim > aligned_size)


def _frozen(case):
    for a in case:
        a.setflags(write=False)
    return case


def _unit(x):
    return (x / np.linalg.norm(x.astype(np.float64), axis=-1, keepdims=True)).astype(np.float32)


def _coordinates(rs, perm):
    """Candidate pixels anywhere in 300 x 300; half of the rows with a planted partner predict it to within 0.9 of the window."""
    cur_uv = rs.uniform(0, 300, size=(perm.size, 2)).astype(np.float32)
    pred_uv = rs.uniform(0, 300, size=(N_REF, 2)).astype(np.float32)
    hit = rs.rand(perm.size) < 0.5
    pred_uv[perm[hit]] = cur_uv[hit] + (rs.uniform(-1, 1, size=(int(hit.sum()), 2)) * np.float32(WINDOW) * 0.9).astype(np.float32)
    return pred_uv, cur_uv


def _planted(dim):
    ref, cur, perm = synth.make_float_descriptors(N_REF, N_CUR, dim=dim, noise=0.25, seed=dim)
    rs = np.random.RandomState(10000 + dim)
    pred_uv, cur_uv = _coordinates(rs, perm)
    return ref, cur, pred_uv, cur_uv


@functools.lru_cache(maxsize=None)
def planted(dim):
    """synth.make_float_descriptors with noise 0.25 (true partner at d ~ 0.015, everything else ~ 0.5) and random pixels."""
    return _frozen(Case(*_planted(dim)))


def _tie_group(rs, ref, cur, pred_uv, cur_uv):
    """Candidates ref_i * s + delta around the (already clustered) TIE_ROWS of ref: candidate k comes from TIE_ROWS[k], scaled by s in
    [0.5, 2] and with relative noise of 1e-6 .. 1e-4 per component, at TIE_SLOTS[k]; two exact duplicates (DUP_LATER, DUP_EARLIER).
    All of them, most inside each other's windows, around pixel (150, 150)."""
    rows, slots = np.array(TIE_ROWS), np.array(TIE_SLOTS)
    for k, slot in enumerate(slots):
        s = np.float32(rs.uniform(0.5, 2.0))
        rel = 10.0 ** rs.uniform(-6, -4)
        cur[slot] = (ref[rows[k]].astype(np.float64) * s * (1.0 + rel * rs.standard_normal(ref.shape[1]))).astype(np.float32)
    cur[DUP_LATER[1]] = cur[slots[DUP_LATER[0]]]
    cur[DUP_EARLIER[1]] = cur[slots[DUP_EARLIER[0]]]
    group = np.concatenate([slots, [DUP_LATER[1], DUP_EARLIER[1]]])
    cur_uv[group] = (np.float32([150, 150]) + rs.uniform(-1, 1, size=(group.size, 2)) * np.float32([50, 40])).astype(np.float32)
    cur_uv[DUP_LATER[1]] = cur_uv[slots[DUP_LATER[0]]]      # a duplicate shares its original's pixel: both or neither in a window
    cur_uv[DUP_EARLIER[1]] = cur_uv[slots[DUP_EARLIER[0]]]
    pred_uv[rows] = (np.float32([150, 150]) + rs.uniform(-15, 15, size=(rows.size, 2))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def near_ties(dim):
    """planted(dim) with the TIE_ROWS of ref pulled into one cluster (a common unit vector plus an offset of length 0.001 .. 0.003) and
    the group of _tie_group planted on them.  For every clustered row the 30 + 2 candidates lie within about 1e-5 of its minimum, a
    row's neighbours in the sorted order 1e-6 or less apart — far inside the shortlist margin, far below what the fp16 copies
    resolve (5e-4), so the approximate order of the group is noise and only the exact side can decide.  Rows TIE_ROWS[:30] have their
    own scaled copy at d ~ 0 +- a few ulp."""
    ref, cur, pred_uv, cur_uv = _planted(dim)
    rs = np.random.RandomState(20000 + dim)
    base = _unit(rs.standard_normal(dim))
    offsets = _unit(rs.standard_normal((len(TIE_ROWS), dim))) * rs.uniform(0.001, 0.003, size=(len(TIE_ROWS), 1)).astype(np.float32)
    ref[list(TIE_ROWS)] = _unit(base[None, :] + offsets)
    _tie_group(rs, ref, cur, pred_uv, cur_uv)
    return _frozen(Case(ref, cur, pred_uv, cur_uv))


def _tails(rs, n, dim):
    """Rows of magnitude 1e-5 .. 5e-5 per component, random signs."""
    return (rs.uniform(1e-5, 5e-5, size=(n, dim)) * rs.choice([-1.0, 1.0], size=(n, dim))).astype(np.float32)


def _heavy(rs):
    """8 components of order 0.35 (0.28 .. 0.42: a norm of about 1), random signs."""
    return 0.35 * rs.uniform(0.8, 1.2, size=8) * rs.choice([-1.0, 1.0], size=8)


@functools.lru_cache(maxsize=None)
def heavy_tail(dim):
    """The input that stresses the subnormal term of the error budget: after normalisation all but 8 components of every row are below
    2^-14, i.e. fp16 subnormals (or zero).  Reference rows with their heavy components at random places; candidate j is row
    (7919 j) mod n_ref with its heavy components off by 10 % and a fresh tail; the TIE_ROWS share one set of heavy components (off by
    1 % from row to row) with tails of their own, and carry the near-tie group of _tie_group."""
    assert dim >= HEAVY_TAIL_MIN_DIM
    rs = np.random.RandomState(30000 + dim)
    ref, cur = _tails(rs, N_REF, dim), _tails(rs, N_CUR, dim)
    places = [rs.choice(dim, size=8, replace=False) for _ in range(N_REF)]
    shared_places, shared = rs.choice(dim, size=8, replace=False), _heavy(rs)
    for i in range(N_REF):
        if i in TIE_ROWS:
            places[i] = shared_places
            ref[i, places[i]] = (shared * (1.0 + 0.01 * rs.standard_normal(8))).astype(np.float32)
        else:
            ref[i, places[i]] = _heavy(rs).astype(np.float32)
    perm = (7919 * np.arange(N_CUR, dtype=np.int64)) % N_REF
    for j in range(N_CUR):
        at = places[perm[j]]
        cur[j, at] = (ref[perm[j], at] * (1.0 + 0.1 * rs.standard_normal(8))).astype(np.float32)
    pred_uv, cur_uv = _coordinates(rs, perm)
    _tie_group(rs, ref, cur, pred_uv, cur_uv)
    return _frozen(Case(np.ascontiguousarray(ref), np.ascontiguousarray(cur), pred_uv, cur_uv))


@functools.lru_cache(maxsize=None)
def irregular(dim, beyond_cap=False):
    """The rows of test_irregular_descriptors (tests/test_float_matcher_gpu.py) at this width: zero, NaN, inf, and scales at which the
    squares overflow, underflow, or leave the regular range of norms.  beyond_cap: 70 further zero candidates, more than the side list
    of irregular candidates holds (kCosineIrregularCap), so that every row takes the exact scan."""
    ref, cur, pred_uv, cur_uv = _planted(dim)
    ref[3] = 0.0
    ref[7, 5 % dim] = np.nan
    ref[11] *= np.float32(1e25)
    ref[13] *= np.float32(1e-30)
    ref[17] *= np.float32(1e15)
    cur[2] = 0.0
    cur[9, 100 % dim] = np.inf
    cur[21] *= np.float32(1e-25)
    cur[40] *= np.float32(3e14)
    if beyond_cap:
        cur[100:170] = 0.0
    return _frozen(Case(ref, cur, pred_uv, cur_uv))


def irregular_rows(x):
    """Rows whose fp32 norm is zero, non-finite or outside [2^-40, 2^40] (what the prep kernels call irregular)."""
    with np.errstate(all="ignore"):
        norm = np.sqrt((x.astype(np.float32) ** 2).sum(axis=1, dtype=np.float32))
        return ~((norm >= np.float32(2.0 ** -40)) & (norm <= np.float32(2.0 ** 40)))


@functools.lru_cache(maxsize=None)
def overflow(dim):
    """12 distinct candidates tiled 100 times (n_cur 1200): every row's best candidate has 100 exact copies, more than a row's
    candidate list holds (kCosineCandCap), and the lowest index must win."""
    ref, cur, _ = synth.make_float_descriptors(N_REF, 12, dim=dim, noise=0.25, seed=dim)
    cur = np.ascontiguousarray(np.tile(cur, (100, 1)))
    rs = np.random.RandomState(40000 + dim)
    cur_uv = rs.uniform(0, 300, size=(cur.shape[0], 2)).astype(np.float32)
    pred_uv = rs.uniform(0, 300, size=(N_REF, 2)).astype(np.float32)
    return _frozen(Case(ref, cur, pred_uv, cur_uv))


def distances64(ref, cur):
    """0.5 - 0.5 cos in float64 from the fp32 inputs, (n_ref, n_cur)."""
    r, c = ref.astype(np.float64), cur.astype(np.float64)
    with np.errstate(all="ignore"):
        return 0.5 - 0.5 * (r @ c.T) / np.linalg.norm(r, axis=1)[:, None] / np.linalg.norm(c, axis=1)[None, :]
