"""A numpy restatement of masked Harris selection and of the track table's retire and fill: TEST INFRASTRUCTURE, never
imported by the package.  The floats are the oracle's (``oracle_lib.harris_response``); everything here is integer logic on top of them,
written for reading, composed with the oracle's trackers by the tests.  ``mutant`` names one deliberate mistake
(tests/test_track_table_ref_cpu.py shows that each is caught)."""
from fractions import Fraction

import numpy as np

from tests import oracle_lib

BORDER = 11
NOT_TRACKED, TRACKED, LARGE_RESIDUAL, OUTSIDE, NUMERIC_ERROR = range(5)
MUTANTS = ("blocked_compete", "reach_off_by_one", "stamp_truncate", "free_retire_order", "next_id_by_n_free")


def survivor_bound(rows, cols, min_distance):
    d = max(int(min_distance), 1)
    return -(-rows // d) * -(-cols // d) if rows >= 2 * BORDER + 1 and cols >= 2 * BORDER + 1 else 0


def stamps(occupied, mask, rows, cols, mutant=None):
    """The pixels (col, row) the occupied points stamp: clamp(floor(x + 0.5), 0, W - 1) in float32, read where the mask byte is not 0."""
    out = []
    if occupied is None:
        return out
    occupied = np.asarray(occupied, np.float32).reshape(-1, 2)
    for i, (x, y) in enumerate(occupied):
        if mask is not None and mask[i] == 0:
            continue
        if mutant == "stamp_truncate":
            fx, fy = np.trunc(x), np.trunc(y)
        else:
            fx, fy = np.floor(np.float32(x) + np.float32(0.5)), np.floor(np.float32(y) + np.float32(0.5))
        fx = 0.0 if np.isnan(fx) else min(max(float(fx), 0.0), float(cols - 1))
        fy = 0.0 if np.isnan(fy) else min(max(float(fy), 0.0), float(rows - 1))
        out.append((int(fx), int(fy)))
    return out


def _sortable(resp):
    bits = resp.view(np.uint32).astype(np.uint64)
    return np.where(bits & np.uint64(0x80000000), ~bits & np.uint64(0xFFFFFFFF), bits | np.uint64(0x80000000))


def _window_max(key, reach):
    """max over the (2 reach + 1)^2 window, clipped at the image."""
    rows, cols = key.shape
    out = key.copy()
    for k in range(1, reach + 1):
        out[:, k:] = np.maximum(out[:, k:], key[:, :cols - k]) if k < cols else out[:, k:]
        out[:, :cols - k] = np.maximum(out[:, :cols - k], key[:, k:]) if k < cols else out[:, :cols - k]
    wide = out.copy()
    for k in range(1, reach + 1):
        if k < rows:
            wide[k:, :] = np.maximum(wide[k:, :], out[:rows - k, :])
            wide[:rows - k, :] = np.maximum(wide[:rows - k, :], out[k:, :])
    return wide


def masked_survivors(image, min_distance, min_response, occupied=None, mask=None, mutant=None):
    """Every survivor as an [S, 2] float32 array of (col, row), strongest first (response descending, then pixel index ascending)."""
    image = np.ascontiguousarray(image, np.uint8)
    rows, cols = image.shape
    if rows < 2 * BORDER + 1 or cols < 2 * BORDER + 1:
        return np.zeros((0, 2), np.float32)
    resp = oracle_lib.harris_response(image)
    reach = max(int(min_distance), 1) - 1
    valid = np.zeros((rows, cols), bool)
    valid[BORDER:rows - BORDER, BORDER:cols - BORDER] = True
    candidate = valid & (resp > np.float32(min_response))
    blocked = np.zeros((rows, cols), bool)
    block_reach = reach + 1 if mutant == "reach_off_by_one" else reach
    for c, r in stamps(occupied, mask, rows, cols, mutant):
        blocked[max(r - block_reach, 0):r + block_reach + 1, max(c - block_reach, 0):c + block_reach + 1] = True
    index = np.arange(rows * cols, dtype=np.uint64).reshape(rows, cols)
    key = (_sortable(resp) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - index)
    competing = candidate if mutant == "blocked_compete" else candidate & ~blocked  # a blocked candidate does not compete
    key = np.where(competing, key, np.uint64(0))
    survives = competing & ~blocked & (key == _window_max(key, reach))
    keys = np.sort(key[survives])[::-1]
    idx = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    return np.stack([(idx % cols).astype(np.float32), (idx // cols).astype(np.float32)], axis=1).reshape(-1, 2)


def detect(image, max_count, min_distance, min_response, occupied=None, mask=None, mutant=None):
    """(uv [max_count, 2] with zeros behind the rows, count) as ftk_harris_detect_device writes them."""
    s = masked_survivors(image, min_distance, min_response, occupied, mask, mutant)
    n = min(len(s), int(max_count))
    uv = np.zeros((int(max_count), 2), np.float32)
    uv[:n] = s[:n]
    return uv, n


def _round_f32(x: Fraction) -> np.float32:
    """x correctly rounded to float32 (nearest, ties to even)."""
    c = np.float32(float(x))
    best = None
    for cand in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - x)
        even = (int(np.float32(cand).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[2]):
            best = (err, cand, even)
    return np.float32(best[1])


def fb_error2(back, start):
    """fmaf(dy, dy, dx * dx) in float32, d = back - start: dx * dx rounded, then dy * dy + that rounded once."""
    dx = np.float32(back[0]) - np.float32(start[0])
    dy = np.float32(back[1]) - np.float32(start[1])
    if not (np.isfinite(dx) and np.isfinite(dy)):
        return np.float32(np.nan)
    p = np.float32(dx * dx)
    if not np.isfinite(p):
        return p
    return _round_f32(Fraction(float(dy)) * Fraction(float(dy)) + Fraction(float(p)))


class Table:
    """The seven tensors of the track table, as numpy arrays, and the free list between retire and fill."""

    def __init__(self, n, next_id=0):
        self.n = int(n)
        self.next_id = np.array([next_id], np.int64)
        self.empty()

    def empty(self):
        n = self.n
        self.ids = np.full(n, -1, np.int64)
        self.points = np.zeros((n, 2), np.float32)
        self.prev_points = np.zeros((n, 2), np.float32)
        self.status = np.full(n, OUTSIDE, np.uint8)
        self.age = np.zeros(n, np.int32)
        self.n_live = np.zeros(1, np.int32)
        self.free = list(range(n))

    def tensors(self):
        return dict(ids=self.ids, points=self.points, prev_points=self.prev_points, status=self.status, age=self.age, n_live=self.n_live,
                    next_id=self.next_id)

    def retire(self, tracked_uv, tracked_status, back_uv=None, back_status=None, fb_threshold=None, mutant=None):
        """After the tracker call(s) over all slots with ref = cur_in = points."""
        t2 = None if back_uv is None else np.float32(fb_threshold) * np.float32(fb_threshold)
        was_free, retired = [s for s in range(self.n) if self.ids[s] < 0], []
        for s in range(self.n):
            if self.ids[s] < 0:
                continue  # an empty slot is not touched
            old, st = self.points[s].copy(), int(tracked_status[s])
            live = st == TRACKED
            if live and back_uv is not None and not (int(back_status[s]) == TRACKED and fb_error2(back_uv[s], old) <= t2):
                live, st = False, LARGE_RESIDUAL
            self.points[s] = tracked_uv[s]
            self.status[s] = st
            if live:
                self.prev_points[s] = old
                self.age[s] += 1
            else:
                self.ids[s] = -1
                retired.append(s)
        self.free = was_free + retired if mutant == "free_retire_order" else sorted(was_free + retired)
        self.n_live[0] = self.n - len(self.free)
        return self.free

    def occupied(self):
        return self.points, (self.ids >= 0).astype(np.uint8)

    def fill(self, survivors, mutant=None):
        """Survivor r < n_free into slot free[r]."""
        n_free = len(self.free)
        filled = min(n_free, len(survivors))
        for r in range(filled):
            s = self.free[r]
            self.ids[s] = self.next_id[0] + r
            self.points[s] = survivors[r]
            self.prev_points[s] = survivors[r]
            self.status[s] = NOT_TRACKED
            self.age[s] = 0
        self.next_id[0] += n_free if mutant == "next_id_by_n_free" else filled
        self.n_live[0] += filled
        self.free = self.free[filled:]
        return filled

    def detect_and_fill(self, image, min_distance, min_response, mutant=None):
        pts, mask = self.occupied()
        return self.fill(masked_survivors(image, min_distance, min_response, pts, mask, mutant), mutant)


def track_frame(table, model, prev_levels, cur_levels, image, min_distance, min_response, forward_backward=None, prior=None, consider_luminance=False,
                **klt_options):
    """One steady-state frame of KltVideoTracker on the oracle's trackers: forward call over all slots from their points, the backward call
    from the results when asked, retire, masked detection on ``image`` (= cur_levels[0]), fill."""
    kw = dict(prior=prior, consider_luminance=consider_luminance, max_points=max(table.n, 1), **klt_options)
    _, uv, st, _ = oracle_lib.klt_track_pyramid(model, prev_levels, cur_levels, table.points, table.points.copy(), table.status.copy(), **kw)
    back_uv = back_st = None
    if forward_backward is not None:
        _, back_uv, back_st, _ = oracle_lib.klt_track_pyramid(model, cur_levels, prev_levels, uv, uv.copy(), st.copy(), **kw)
    table.retire(uv, st, back_uv, back_st, forward_backward)
    table.detect_and_fill(image, min_distance, min_response)
    return uv, st, back_uv, back_st
