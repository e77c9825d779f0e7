"""hamming_ref for the Hamming matcher: a restatement of the reference's DescriptorMatcher<BriefType> ForceMatch / NearbyMatch
(descriptor_matcher.h) and of the BRIEF ComputeDistance of its caller (test/test_descriptor_matcher_brief.cpp:33-45) in whole-array numpy.

TEST INFRASTRUCTURE ONLY.  Written from the reference's source (file:line below, descriptor_matcher.h unless another file is named),
independently of oracle/oracle_matcher.c and of the kernels: it imports numpy and the standard library only and shares no line with
tests/oracle_lib.py, with oracle/ or with the package.

Domain: descriptors are per-bit arrays (n, n_bits) uint8 holding 0 or 1 (BriefType is a container of bits; a kernel sees them packed,
this module never packs).  Everything the reference does in `float` is done in float32: the distance is an int32 count cast to float
(test_descriptor_matcher_brief.cpp:44), the threshold is the `float` member kMaxValidDescriptorDistance (:19), the window bounds are
the int32 members (:17-18) converted to float by the comparison, the coordinates are Vec2 of float.

  distance_pair(a, b)                      ComputeDistance of one pair, as written                 test_descriptor_matcher_brief.cpp:33-45
  distances(ref, cur)                      the same for all pairs, (n_ref, n_cur) float32, in row blocks
  window(pred_uv, cur_uv, col, row)        True where the pair is NOT skipped by :108-111
  select(D, ok, max_distance, stale)       the running-best rule of :67-76 / :105-121 on a distance matrix
  force_match / nearby_match               the two overloads, with their return conventions        :55-79 / :90-124
  scan_literal(...)                        the same two loops written pair by pair (slow; the tests hold select() to it)

The count of differing bits of all pairs is taken as a . (1 - b) + (1 - a) . b, two matrix products in float32: every term is 0 or 1
and every partial sum is an integer of at most n_bits < 2^24, so the products are exact whatever order the BLAS sums in.

The rule, :68-75 and :106-117: min_distance starts AT the threshold and a candidate replaces the running best iff
`distance < min_distance && distance < threshold`: the lowest j among the candidates of minimum distance, and only if that minimum is
below the threshold.  index_pairs is reset to -1 only when its size differs from descriptors_ref (:60-62, :98-100); an entry without a
match keeps what it held.  NearbyMatch leaves a row's scan at the first candidate of distance 0 (:119); no later candidate could have
replaced it (strict '<'), so the break changes no result: scan_literal keeps it, select() has no need of it.

`Flags` carries the mutants: each switch introduces ONE plausible misreading, so that a test can show that its criterion fails on it.

sweep_case() builds the inputs that tests/test_hamming_ref_cpu.py and tests/test_matcher_widths_gpu.py share.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

f32 = np.float32
K_MAX_INT32 = f32(2147483647)  # kMaxInt32 through `return kMaxInt32` of a float function: 2^31 (test_descriptor_matcher_brief.cpp:34-36)
ROW_BLOCK = 256                # reference rows per block of distances()


@dataclasses.dataclass(frozen=True)
class Flags:
    """Mutants, each off by default."""
    le_threshold: bool = False        # distance <= kMaxValidDescriptorDistance accepted (:71, :114)
    highest_j_on_ties: bool = False   # `<=` against the running minimum: the LAST candidate of the minimum wins (:71, :114)
    window_ge: bool = False           # skipped when |d| >= the bound, not > (:108-109)
    nan_fails_window: bool = False    # written as "kept iff |du| <= col && |dv| <= row": NaN is skipped (:108-111)
    always_reset: bool = False        # index_pairs assigned -1 whatever its size (:60-62, :98-100)
    padded_count: bool = False        # distance over whole 32-bit words whose pad bits are not zero (a kernel counting its padding)


DEFAULT = Flags()


# ---- ComputeDistance (test_descriptor_matcher_brief.cpp:33-45) ---------------------------------------------------------------------

def distance_pair(a, b) -> np.float32:
    """One pair, as written: kMaxInt32 for an empty descriptor, else the number of positions that differ."""
    a, b = np.asarray(a), np.asarray(b)
    if a.size == 0 or b.size == 0:
        return K_MAX_INT32
    return f32(int(np.count_nonzero(a != b[: a.size])))


def _bits(x):
    x = np.asarray(x)
    if x.ndim != 2:
        x = x.reshape(x.shape[0], -1) if x.size else x.reshape(x.shape[0] if x.ndim else 0, 0)
    if x.size and int(x.max()) > 1:
        raise ValueError("hamming_ref: descriptors hold 0 / 1")
    return x.astype(np.uint8)


def _with_pad(bits, odd_rows_set):
    """padded_count: the rows extended to whole 32-bit words; the pad bits are 1 in the odd rows of `cur`, 0 elsewhere."""
    n, n_bits = bits.shape
    pad = -n_bits % 32
    ext = np.zeros((n, pad), np.uint8)
    if odd_rows_set:
        ext[1::2] = 1
    return np.concatenate([bits, ext], axis=1)


def distances(ref_bits, cur_bits, flags: Flags = DEFAULT) -> np.ndarray:
    """(n_ref, n_cur) float32: ComputeDistance of every pair, ROW_BLOCK reference rows at a time."""
    ref, cur = _bits(ref_bits), _bits(cur_bits)
    n_ref, n_cur = ref.shape[0], cur.shape[0]
    if ref.shape[1] == 0 or cur.shape[1] == 0:
        return np.full((n_ref, n_cur), K_MAX_INT32, f32)
    if flags.padded_count:
        ref, cur = _with_pad(ref, False), _with_pad(cur, True)
    b = cur.astype(f32).T          # (n_bits, n_cur)
    not_b = f32(1) - b
    out = np.empty((n_ref, n_cur), f32)
    for r0 in range(0, n_ref, ROW_BLOCK):
        a = ref[r0:r0 + ROW_BLOCK].astype(f32)
        out[r0:r0 + ROW_BLOCK] = a @ not_b + (f32(1) - a) @ b
    return out


# ---- the window of NearbyMatch (:108-111) ----------------------------------------------------------------------------------------------

def window(pred_uv, cur_uv, max_col: int, max_row: int, flags: Flags = DEFAULT) -> np.ndarray:
    """(n_ref, n_cur) bool: True where the candidate is looked at.  Skipped iff |du| > col || |dv| > row in float32; a NaN difference
    compares false, so it is looked at."""
    pred = np.asarray(pred_uv, f32).reshape(-1, 2)
    cur = np.asarray(cur_uv, f32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        du = np.abs(pred[:, None, 0] - cur[None, :, 0])
        dv = np.abs(pred[:, None, 1] - cur[None, :, 1])
        col, row = f32(int(max_col)), f32(int(max_row))
        if flags.nan_fails_window:
            return (du <= col) & (dv <= row)
        if flags.window_ge:
            return ~((du >= col) | (dv >= row))
        return ~((du > col) | (dv > row))


# ---- the running best (:67-76, :105-121) -----------------------------------------------------------------------------------------------

def _start(n_ref, index_pairs, flags):
    """:60-62 / :98-100."""
    if index_pairs is None or flags.always_reset:
        return np.full(n_ref, -1, np.int32)
    held = np.asarray(index_pairs, np.int32).reshape(-1)
    return held.copy() if held.size == n_ref else np.full(n_ref, -1, np.int32)


def select(D, looked_at, max_distance, index_pairs=None, flags: Flags = DEFAULT) -> np.ndarray:
    """index_pairs after the loops, from the distances D (n_ref, n_cur) float32 and the mask of candidates that are looked at (None: all)."""
    n_ref, n_cur = D.shape
    out = _start(n_ref, index_pairs, flags)
    if n_ref == 0 or n_cur == 0:
        return out
    thr = f32(max_distance)
    E = D if looked_at is None else np.where(looked_at, D, f32(np.inf))
    if flags.highest_j_on_ties:
        j = (n_cur - 1 - np.argmin(E[:, ::-1], axis=1)).astype(np.int32)
    else:
        j = np.argmin(E, axis=1).astype(np.int32)  # the first occurrence of the minimum
    best = E[np.arange(n_ref), j]
    found = (best <= thr) if flags.le_threshold else (best < thr)
    found &= np.isfinite(best)  # (a row whose every candidate was skipped)
    out[found] = j[found]
    return out


def scan_literal(ref_bits, cur_bits, max_distance, index_pairs=None, pred_uv=None, cur_uv=None, max_col=40, max_row=40) -> np.ndarray:
    """The loops of :67-76 (pred_uv None) / :105-121 pair by pair, unmutated.  For small inputs."""
    ref, cur = _bits(ref_bits), _bits(cur_bits)
    out = _start(ref.shape[0], index_pairs, DEFAULT)
    thr = f32(max_distance)
    if pred_uv is not None:
        pred, cuv = np.asarray(pred_uv, f32).reshape(-1, 2), np.asarray(cur_uv, f32).reshape(-1, 2)
    for i in range(ref.shape[0]):
        min_distance = thr
        for j in range(cur.shape[0]):
            if pred_uv is not None:
                with np.errstate(invalid="ignore"):
                    if abs(f32(pred[i, 0] - cuv[j, 0])) > f32(int(max_col)) or abs(f32(pred[i, 1] - cuv[j, 1])) > f32(int(max_row)):
                        continue
            distance = distance_pair(ref[i], cur[j])
            if distance < min_distance and distance < thr:
                min_distance = distance
                out[i] = j
            if pred_uv is not None and distance == 0:
                break
    return out


# ---- ForceMatch / NearbyMatch -----------------------------------------------------------------------------------------------------------

def _unchanged(index_pairs):
    """What the caller's vector holds after an early `return false`: what it held."""
    held = [] if index_pairs is None else index_pairs
    return np.array(held, dtype=np.int32).reshape(-1)


def force_match(ref_bits, cur_bits, max_distance, index_pairs=None, flags: Flags = DEFAULT, D=None):
    """(ok, index_pairs_in_cur).  :58 — no candidates: false, index_pairs untouched.  `D`: distances() of the same inputs, if at hand."""
    ref, cur = _bits(ref_bits), _bits(cur_bits)
    if cur.shape[0] == 0:
        return False, _unchanged(index_pairs)
    D = distances(ref, cur, flags) if D is None else D
    return True, select(D, None, max_distance, index_pairs, flags)


def nearby_match(ref_bits, cur_bits, pred_uv, cur_uv, max_distance, max_col=40, max_row=40, index_pairs=None, flags: Flags = DEFAULT, D=None):
    """(ok, index_pairs_in_cur).  :94-96 — no candidates, or a coordinate list of another length: false, index_pairs untouched."""
    ref, cur = _bits(ref_bits), _bits(cur_bits)
    pred = np.asarray(pred_uv, f32).reshape(-1, 2)
    cuv = np.asarray(cur_uv, f32).reshape(-1, 2)
    if cur.shape[0] == 0 or ref.shape[0] != pred.shape[0] or cur.shape[0] != cuv.shape[0]:
        return False, _unchanged(index_pairs)
    D = distances(ref, cur, flags) if D is None else D
    return True, select(D, window(pred, cuv, max_col, max_row, flags), max_distance, index_pairs, flags)


# ---- the inputs of the width-and-shape sweep -------------------------------------------------------------------------------------------

SWEEP_BITS = (1, 31, 32, 33, 65, 96, 127, 129, 250, 257, 300, 480, 511, 513, 544, 768, 1000, 2048)
SWEEP_SHAPES = ((65, 33), (130, 95), (513, 1001))
SWEEP_WINDOW = (35, 80)  # (kMaxValidPredictColDistance, kMaxValidPredictRowDistance) of the sweep's NearbyMatch


def sweep_params():
    """(n_bits, n_ref, n_cur) of the sweep: above 512 bits the first two shapes only."""
    return [(b, r, c) for b in SWEEP_BITS for (r, c) in SWEEP_SHAPES if b <= 512 or (r, c) != SWEEP_SHAPES[-1]]


@dataclasses.dataclass
class Case:
    n_bits: int
    flips: int
    ref: np.ndarray       # (n_ref, n_bits) uint8
    cur: np.ndarray       # (n_cur, n_bits) uint8
    pred_uv: np.ndarray   # (n_ref, 2) float32
    cur_uv: np.ndarray    # (n_cur, 2) float32
    stale: np.ndarray     # (n_ref,) int32, arange + 7000
    partner: np.ndarray   # (n_cur,) reference row a candidate was planted from, -1: an unrelated candidate
    thresholds: tuple


def planted(rs, n_bits, n_ref, n_cur, flips):
    """Random descriptors; candidate j (j % 3 != 2) is reference row partner[j] with `flips` bits flipped; reference rows i % 4 == 1 have
    no partner.  The first n_partners planted candidates come from distinct rows."""
    ref = rs.randint(0, 2, size=(n_ref, n_bits)).astype(np.uint8)
    cur = rs.randint(0, 2, size=(n_cur, n_bits)).astype(np.uint8)
    rows = np.flatnonzero(np.arange(n_ref) % 4 != 1)
    js = np.flatnonzero(np.arange(n_cur) % 3 != 2)
    stride = next(s for s in range(37, 37 + rows.size + 1) if math.gcd(s, rows.size) == 1)
    partner = np.full(n_cur, -1, np.int64)
    partner[js] = rows[(np.arange(js.size) * stride) % rows.size]
    cur[js] = ref[partner[js]]
    cols = np.argsort(rs.random_sample((js.size, n_bits)), axis=1)[:, :flips]  # `flips` distinct positions per planted candidate
    cur[js[:, None], cols] ^= 1
    return ref, cur, partner


def sweep_case(n_bits: int, n_ref: int, n_cur: int, window=SWEEP_WINDOW) -> Case:
    """One input of the sweep (n_cur >= 24).  Beside the planted partners at distance `flips` = max(1, n_bits // 12):
      * candidate n_cur // 2 is a copy of candidate 3: the lower index must win;
      * reference row 7 and candidate 11 are all zero (distance 0 between them);
      * about half of the partnered rows are predicted within the window of their candidate, the rest anywhere;
      * candidate 4 sits exactly kMaxValidPredictColDistance beside its row's prediction: `>` keeps it, `>=` would not;
      * the row of candidate 6 has NaN in its predicted u, and candidate 9 has NaN in its v while its row is predicted far outside the
        image: both pairs are looked at only because NaN passes the window test;
      * stale indices arange + 7000."""
    assert n_cur >= 24 and n_ref >= 24
    rs = np.random.RandomState((1000003 * n_bits + 1009 * n_ref + n_cur) % (2 ** 31))
    flips = max(1, n_bits // 12)
    ref, cur, partner = planted(rs, n_bits, n_ref, n_cur, flips)
    cur[n_cur // 2] = cur[3]
    partner[n_cur // 2] = partner[3]
    ref[7] = 0
    cur[11] = 0
    partner[partner == 7] = -1
    assert (partner[[3, 4, 6, 9]] >= 0).all() and len(set(partner[[3, 4, 6, 9]])) == 4
    col, row = window
    cur_uv = rs.uniform(0, 300, size=(n_cur, 2)).astype(f32)
    pred_uv = rs.uniform(0, 300, size=(n_ref, 2)).astype(f32)
    js = np.flatnonzero(partner >= 0)
    near = js[rs.random_sample(js.size) < 0.5]
    pred_uv[partner[near]] = cur_uv[near] + (rs.uniform(-0.8, 0.8, size=(near.size, 2)) * np.array([col, row])).astype(f32)
    cur_uv[4] = (100.0, 100.0)
    pred_uv[partner[4]] = (100.0 + col, 100.0)
    pred_uv[partner[6]] = (np.nan, cur_uv[6, 1])
    cur_uv[9] = (cur_uv[9, 0], np.nan)
    pred_uv[partner[9]] = (cur_uv[9, 0], 5000.0)
    stale = np.arange(n_ref, dtype=np.int32) + 7000
    return Case(n_bits, flips, ref, cur, pred_uv, cur_uv, stale, partner, (0.0, float(flips), flips + 0.5, 60.0, 3e9))


def assert_case_is_telling(c: Case, D=None, window=SWEEP_WINDOW):
    """The case does what it is there for: under some threshold tried some rows match and some do not (NearbyMatch at every width;
    ForceMatch from 31 bits on: below that unrelated descriptors are as close as planted ones), the duplicate's lower index is an
    answer, the all-zero pair is at distance 0, and from 33 bits on some row's best distance EQUALS a threshold tried."""
    D = distances(c.ref, c.cur) if D is None else D
    mixed_force = mixed_nearby = False
    for thr in c.thresholds:
        f = force_match(c.ref, c.cur, thr, None, D=D)[1]
        with np.errstate(invalid="ignore"):
            n = nearby_match(c.ref, c.cur, c.pred_uv, c.cur_uv, thr, window[0], window[1], None, D=D)[1]
        mixed_force |= bool((f >= 0).any() and (f < 0).any())
        mixed_nearby |= bool((n >= 0).any() and (n < 0).any())
    assert mixed_nearby and (mixed_force or c.n_bits < 31), c.n_bits
    assert D[7, 11] == 0
    if c.n_bits >= 31:
        assert force_match(c.ref, c.cur, c.flips + 0.5, None, D=D)[1][c.partner[3]] == 3 and D[c.partner[3], c.cur.shape[0] // 2] == c.flips
    if c.n_bits >= 33:
        assert np.isin(D.min(axis=1), np.asarray(c.thresholds, f32)).any(), c.n_bits
