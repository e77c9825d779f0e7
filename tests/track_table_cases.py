"""Shared by tests/test_track_table_cases_cpu.py and tests/test_track_table_gpu.py: deterministic table states, tracker outcomes and the
fill image for the track table's retire and fill entries at the slot counts where track_retire_kernel changes its
shape.  numpy only; the expected results come from tests/track_table_ref.py."""
import functools

import numpy as np

from feature_tracker_amd import synth
from tests import track_table_ref as R

RETIRE_BLOCK, RANK_TILE, MAX_SLOTS = 1024, 256, 65536
# 64 513 = 63 * 1024 + 1: 64 slots per thread, owners 0 .. 1007 full, owner 1008 holds one slot, 15 threads own nothing
SIZES = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 64513, 65535, 65536)
FB_SIZES = (2, 1025, 2049)
FB_THRESHOLDS = (0.0, 1.0)
PATTERNS = ("all_live", "all_dead", "alternating", "random", "last_held_dead", "one_live", "owner_runs", "all_empty", "every_status")
STATUS_BYTES = (0, 1, 2, 3, 4, 255)
WIDTH, HEIGHT = 333, 251

# what an empty slot carries, so that "an empty slot is not touched" shows; float words are given as bits
POISON_POINT_BITS, POISON_PREV_BITS, POISON_STATUS, POISON_AGE = 0xDEADBEEF, 0xFEEDFACE, 0xA5, 0x5A5A5A5A
GUARD = 32  # elements of poison before and after every array the kernels write
GUARD_FILL = {"ids": 0x7A7A7A7A7A7A7A7A, "points": 0xCAFEF00D, "prev_points": 0xBADDCAFE, "status": 0xEE, "age": 0x6B6B6B6B, "free_slots": 0x7C7C7C7C,
              "n_live": 0x1D1D1D1D, "n_free": 0x2E2E2E2E, "next_id": 0x3F3F3F3F3F3F3F3F}

# the fill image: the synthetic scene at the size of tests/test_harris_device_gpu.py's largest (its survivor count: tests/test_track_table_cases_cpu.py)
FILL_MIN_DISTANCE, FILL_MIN_RESPONSE = 2, 40.0


def per_thread(n):
    return -(-int(n) // RETIRE_BLOCK)


def owner_of(n):
    """The thread of track_retire_kernel that owns each slot."""
    return np.arange(int(n)) // per_thread(n)


def _rs(n, seed, salt):
    return np.random.RandomState((int(n) * 7919 + int(seed) * 104729 + salt) % (2 ** 31 - 1))


def _per_owner(n, values, probabilities, rs):
    owners = int(owner_of(n)[-1]) + 1
    return rs.choice(values, size=owners, p=probabilities)[owner_of(n)]


def state(n, seed, held="random", quarter_pixels=False):
    """A table of n slots.  ``held``: "random" (about 70 % of the slots hold an id: one owner in eight holds all of its slots, one in
    sixteen none, the others 70 %; the last slot always holds one), "all" or "none".  Ids are distinct, some beyond 2^31; ages are
    random; points lie inside the WIDTH x HEIGHT image (on multiples of 0.25 where asked, so that small offsets add exactly)."""
    n = int(n)
    rs = _rs(n, seed, 1)
    t = R.Table(n, next_id=int(rs.randint(0, 1 << 30)) + (1 << 33))
    if held == "random":
        rate = _per_owner(n, [1.0, 0.0, 0.7], [1 / 8, 1 / 16, 13 / 16], rs)
        holds = rs.uniform(size=n) < rate
        holds[-1] = True
    else:
        holds = np.full(n, held == "all")
    t.ids[:] = np.where(holds, rs.permutation(n).astype(np.int64) + np.where(rs.uniform(size=n) < 0.5, 1 << 32, 0), -1)
    xy = np.stack([rs.uniform(1.0, WIDTH - 2.0, n), rs.uniform(1.0, HEIGHT - 2.0, n)], axis=1)
    old = np.stack([rs.uniform(1.0, WIDTH - 2.0, n), rs.uniform(1.0, HEIGHT - 2.0, n)], axis=1)
    if quarter_pixels:
        xy = np.floor(xy * 4.0) / 4.0
    t.points[:] = xy.astype(np.float32)
    t.prev_points[:] = old.astype(np.float32)
    t.status[:] = rs.choice([R.NOT_TRACKED, R.TRACKED], size=n).astype(np.uint8)
    t.age[:] = rs.randint(0, 1000000000, n).astype(np.int32)
    empty = ~holds
    t.points.view(np.uint32)[empty] = POISON_POINT_BITS
    t.prev_points.view(np.uint32)[empty] = POISON_PREV_BITS
    t.status[empty] = POISON_STATUS
    t.age[empty] = POISON_AGE
    t.n_live[0] = int(holds.sum())
    t.free = None  # retire writes it
    return t


def held_mode(pattern):
    return {"all_empty": "none", "owner_runs": "all"}.get(pattern, "random")


def outcome(table, pattern, seed):
    """tracked_status uint8 [n] for one pattern, dealt over the slots that hold an id.  The bytes of empty slots are random and half of
    them say TRACKED: an empty slot must not come back to life."""
    n = table.n
    rs = _rs(n, seed, 2 + PATTERNS.index(pattern))
    held = np.flatnonzero(table.ids >= 0)
    st = np.where(rs.uniform(size=n) < 0.5, R.TRACKED, rs.choice(STATUS_BYTES, size=n)).astype(np.uint8)
    dead_bytes = rs.choice([R.NOT_TRACKED, R.LARGE_RESIDUAL, R.OUTSIDE, R.NUMERIC_ERROR], size=n).astype(np.uint8)
    dead = np.zeros(n, bool)
    if pattern == "all_live" or pattern == "all_empty":
        pass
    elif pattern == "all_dead":
        dead[held] = True
    elif pattern == "alternating":
        dead[held[1::2]] = True
    elif pattern == "random":  # 30 % on the whole: one owner in four loses nothing, the others 40 %
        dead[held] = (rs.uniform(size=n) < _per_owner(n, [0.0, 0.4], [1 / 4, 3 / 4], rs))[held]
    elif pattern == "last_held_dead":
        dead[held[-1:]] = True
    elif pattern == "one_live":
        dead[held] = True
        dead[held[len(held) // 2:len(held) // 2 + 1]] = False
    elif pattern == "owner_runs":  # whole owners dead next to whole owners live
        dead[held] = (_per_owner(n, [0, 1], [0.5, 0.5], rs) == 1)[held]
    elif pattern == "every_status":
        st[held] = np.resize(np.array(STATUS_BYTES, np.uint8), len(held))[rs.permutation(len(held))]
        return st
    else:
        raise ValueError(pattern)
    st[held] = np.where(dead[held], dead_bytes[held], R.TRACKED)
    return st


def tracked_points(n, seed):
    """Where the tracker left the slots: float32 [n, 2] around the image, a few outside."""
    rs = _rs(n, seed, 40)
    return np.stack([rs.uniform(-3.0, WIDTH + 3.0, int(n)), rs.uniform(-3.0, HEIGHT + 3.0, int(n))], axis=1).astype(np.float32)


HOSTILE_BITS = (0x7FC00000, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x7149F2CA)  # NaNs, +-inf, -0.0, 1e30


def hostile_points(n, seed):
    """tracked_points with NaN (quiet, with a payload, signalling), +-inf, -0.0 and 1e30 sprinkled over a third of the words."""
    uv = tracked_points(n, seed)
    rs = _rs(n, seed, 41)
    words = uv.view(np.uint32).reshape(-1)
    hit = rs.uniform(size=words.size) < 1 / 3
    words[hit] = rs.choice(np.array(HOSTILE_BITS, np.uint32), size=int(hit.sum()))
    return uv


def fb_state(n, seed):
    """The table of the forward-backward cases: quarter-pixel points; at n = 2 both slots hold an id."""
    return state(n, seed, held="random" if n >= RETIRE_BLOCK - 1 else "all", quarter_pixels=True)


FB_KINDS = ("on_the_point", "ulp_beyond_0", "exactly_1", "ulp_beyond_1", "far", "nan", "inf")


def forward_backward(table, seed):
    """(tracked_status, back_uv, back_status, kind [n]) on a quarter-pixel table: every forward status says TRACKED but one slot in
    nine, and the backward results are dealt over FB_KINDS, the same for both thresholds: on the old point (error 0), one ulp off it
    (beyond t = 0), at distance exactly 1 along an axis, one ulp beyond that, far away, NaN, +inf; the backward status says TRACKED
    for two slots in three."""
    n = table.n
    rs = _rs(n, seed, 50)
    slot = np.arange(n)
    kind = slot % len(FB_KINDS)
    back_status = np.where((slot // len(FB_KINDS)) % 3 != 2, R.TRACKED, rs.choice([0, 2, 3, 4, 255], size=n)).astype(np.uint8)
    tracked_status = np.where((slot // (3 * len(FB_KINDS))) % 3 != 2, R.TRACKED, R.OUTSIDE).astype(np.uint8)
    axis = (slot // 2) % 2
    back = table.points.copy()
    up = np.float32(np.inf)
    for s in range(n):
        a, name = axis[s], FB_KINDS[kind[s]]
        if name == "ulp_beyond_0":
            back[s, a] = np.nextafter(back[s, a], up)
        elif name == "exactly_1":
            back[s, a] += np.float32(1.0)
        elif name == "ulp_beyond_1":
            back[s, a] = np.nextafter(back[s, a] + np.float32(1.0), up)
        elif name == "far":
            back[s] += np.float32(17.5)
        elif name == "nan":
            back[s, a] = np.float32(np.nan)
        elif name == "inf":
            back[s, a] = up
    return tracked_status, back, back_status, kind


@functools.lru_cache(maxsize=None)
def fill_image():
    return np.ascontiguousarray(synth.make_image_pair(WIDTH, HEIGHT, (0.0, 0.0))[0])


@functools.lru_cache(maxsize=None)
def fill_survivors():
    """The fill image's survivors with no occupied point, strongest first."""
    return R.masked_survivors(fill_image(), FILL_MIN_DISTANCE, FILL_MIN_RESPONSE)


FILL_MASKING = 96  # live slots that sit on every other one of the strongest survivors


def fill_state(n, n_free, seed):
    """A table of n slots, all but a few holding an id, and the tracker outcome after which exactly n_free slots are empty and the points
    of the live ones are known: FILL_MASKING live slots (fewer when n - n_free is smaller) sit on every other one of the strongest
    survivors of the fill image and block them; the other live slots sit in the image's corner, inside the border band, where a stamp
    of reach min_distance - 1 blocks no candidate.  So the masked survivor count does not depend on n_free, which is then free to be
    chosen around it.  A fifth of the slots that end empty are empty before the call, the rest are retired by it.
    Returns (table, tracked_uv, tracked_status)."""
    n, n_free = int(n), int(n_free)
    rs = _rs(n, seed + n_free, 60)
    t = state(n, seed + n_free, held="all")
    order = rs.permutation(n)
    ends_empty, stays = order[:n_free], order[n_free:]
    masking = stays[:FILL_MASKING]
    strongest = fill_survivors()[0:2 * len(masking):2]
    corner = np.stack([rs.uniform(0.0, 8.0, n), rs.uniform(0.0, 8.0, n)], axis=1).astype(np.float32)
    t.points[stays] = corner[stays]
    t.points[masking[:len(strongest)]] = strongest + rs.uniform(-0.45, 0.45, strongest.shape).astype(np.float32)  # rounds to the survivor's pixel
    before = ends_empty[:n_free // 5]
    t.ids[before] = -1
    t.points.view(np.uint32)[before] = POISON_POINT_BITS
    t.prev_points.view(np.uint32)[before] = POISON_PREV_BITS
    t.status[before] = POISON_STATUS
    t.age[before] = POISON_AGE
    t.n_live[0] = n - len(before)
    tracked_uv = t.points.copy()  # live slots stay where they are
    tracked_uv[ends_empty] = hostile_points(n, seed)[ends_empty]
    tracked_status = np.full(n, R.TRACKED, np.uint8)
    tracked_status[ends_empty] = rs.choice([0, 2, 3, 4, 255], size=n_free).astype(np.uint8)
    tracked_status[before] = R.TRACKED
    return t, tracked_uv, tracked_status


def fill_free_counts(n, masked_count):
    """The free-list lengths of test_fill_across_rank_tiles for a table of n slots: around the rank tile and around the masked survivor count."""
    return sorted({c for c in (0, 1, RANK_TILE - 1, RANK_TILE, RANK_TILE + 1, masked_count - 1, masked_count, masked_count + 3) if 0 <= c <= n})
