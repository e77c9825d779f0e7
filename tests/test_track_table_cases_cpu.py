"""The conditions tests/test_track_table_gpu.py relies on, established on the CPU: the generators of tests/track_table_cases.py reach the
shapes of track_retire_kernel (1, 2, 3 and 64 slots per thread, a partial last owner, idle threads, bit 63 of the dead mask, counts
above 1 in the scan), the forward-backward cases sit on both sides of both thresholds, and the fill image has more survivors than
three rank tiles.

The fill image is the synthetic 333 x 251 scene at min_distance 2, min_response 40.0: S = 1 650 survivors with no occupied point
(six full tiles of 256 and 114 more), 1 812 once FILL_MASKING live slots sit on every other one of the strongest (a blocked corner does
not compete, so its neighbours come through)."""
import numpy as np
import pytest

from tests import track_table_cases as C
from tests import track_table_ref as R

S_RECORDED, S_MASKED_RECORDED = 1650, 1812


def _retired(n, pattern, seed=0):
    """(dead as the kernel counts it: empty before or retired now, the table after, its free list)."""
    t = C.state(n, seed, C.held_mode(pattern))
    free = t.retire(C.tracked_points(n, seed), C.outcome(t, pattern, seed))
    dead = np.zeros(n, bool)
    dead[free] = True
    return dead, t, free


def test_sizes_reach_every_owner_shape():
    assert sorted({C.per_thread(n) for n in C.SIZES}) == [1, 2, 3, 64]
    assert C.SIZES[-1] == C.MAX_SLOTS and set(C.FB_SIZES) <= set(C.SIZES)
    owners = C.owner_of(64513)
    assert owners[-1] == 1008 and (owners == 1008).sum() == 1 and (owners == 1007).sum() == 64  # a partial last owner, 15 idle threads
    assert C.owner_of(65536)[-1] == 1023 and C.owner_of(1023)[-1] == 1022 and C.owner_of(2049)[-1] == 682


@pytest.mark.parametrize("n", C.SIZES)
def test_states_are_what_they_say(n):
    t = C.state(n, 0)
    held = t.ids >= 0
    assert held[-1] and len(set(t.ids[held].tolist())) == held.sum() and int(t.n_live[0]) == held.sum()
    if n >= 1023:
        assert 0.6 < held.mean() < 0.8 and (t.ids > 1 << 31).any()
    assert (t.points.view(np.uint32)[~held] == C.POISON_POINT_BITS).all() and (t.status[~held] == C.POISON_STATUS).all()
    assert (t.points[held] >= 0).all() and (t.points[held, 0] <= C.WIDTH - 1).all() and (t.points[held, 1] <= C.HEIGHT - 1).all()
    assert not (C.state(n, 0, "none").ids >= 0).any() and (C.state(n, 0, "all").ids >= 0).all()
    for pattern in C.PATTERNS:
        t = C.state(n, 0, C.held_mode(pattern))
        st, held = C.outcome(t, pattern, 0), t.ids >= 0
        assert st.dtype == np.uint8 and st.shape == (n,)
        if n >= 1023 and pattern != "owner_runs":
            assert (st[~held] == R.TRACKED).any()  # an empty slot whose tracker byte says TRACKED stays empty
        if pattern == "every_status" and held.sum() >= 6:
            assert set(st[held].tolist()) == set(C.STATUS_BYTES)


@pytest.mark.parametrize("n", C.SIZES)
def test_patterns_reach_the_scan_and_the_mask(n):
    k, owners = C.per_thread(n), C.owner_of(n)
    dead, t, free = _retired(n, "random")
    per_owner = np.bincount(owners, weights=dead, minlength=owners[-1] + 1).astype(int)
    assert free == sorted(free) and (0 < len(free) < n or n <= 2)
    if k >= 2:
        assert (per_owner >= 2).any() and (per_owner == 0).any()  # counts above 1 flow through the scan next to zeros
        assert (per_owner[:-1] == k).any() or k == 64  # (a whole owner dead: the owners that hold nothing)
    runs, _, _ = _retired(n, "owner_runs")
    full = np.bincount(owners, weights=runs, minlength=owners[-1] + 1).astype(int)
    if n >= 1023:
        size = np.bincount(owners)
        assert (full == size).any() and (full == 0).any() and set(full.tolist()) <= {0} | set(size.tolist())
    if n == 65536:
        assert dead.reshape(1024, 64)[:, 63].any() and not dead.reshape(1024, 64)[:, 63].all()  # the shift by 63
        assert runs.reshape(1024, 64)[:, 63].any()
    if n == 64513:
        last = {p: bool(_retired(n, p)[0][64512]) for p in C.PATTERNS}
        assert last["last_held_dead"] and last["all_dead"] and not last["all_live"]  # the partial owner's one slot, dead here and live there
    counts = {p: len(_retired(n, p)[2]) for p in C.PATTERNS}
    assert counts["all_dead"] == n and counts["all_empty"] == n
    if n >= 1023:
        assert counts["one_live"] == n - 1 and counts["all_live"] < counts["last_held_dead"] < counts["random"] < n


@pytest.mark.parametrize("n", C.FB_SIZES)
def test_forward_backward_cases_sit_on_both_sides_of_both_thresholds(n):
    verdicts = {}
    for t in C.FB_THRESHOLDS:
        table = C.fb_state(n, 0)
        tracked_status, back_uv, back_status, kind = C.forward_backward(table, 0)
        table.retire(table.points + np.float32(0.25), tracked_status, back_uv, back_status, t)
        verdicts[t] = table.ids >= 0
    table = C.fb_state(n, 0)
    held = table.ids >= 0
    ok = held & (tracked_status == R.TRACKED) & (back_status == R.TRACKED)
    of = {name: ok & (kind == i) for i, name in enumerate(C.FB_KINDS)}
    if n == 2:  # two slots: the point itself and one ulp off it
        assert verdicts[0.0].tolist() == [True, False] and verdicts[1.0].tolist() == [True, True]
        return
    assert (verdicts[0.0] != verdicts[1.0]).any()
    for name in C.FB_KINDS:
        assert of[name].sum() >= 3, name
    assert verdicts[0.0][of["on_the_point"]].all() and not verdicts[0.0][of["ulp_beyond_0"]].any()  # exactly t^2 against one ulp beyond, t = 0
    assert verdicts[1.0][of["exactly_1"]].all() and not verdicts[1.0][of["ulp_beyond_1"]].any()  # and t = 1
    assert verdicts[1.0][of["ulp_beyond_0"]].all() and not verdicts[0.0][of["exactly_1"]].any()
    for t in C.FB_THRESHOLDS:
        assert not verdicts[t][of["far"] | of["nan"] | of["inf"]].any()
        assert not verdicts[t][held & ((tracked_status != R.TRACKED) | (back_status != R.TRACKED))].any()
    assert (held & (tracked_status != R.TRACKED)).any() and (held & (tracked_status == R.TRACKED) & (back_status != R.TRACKED)).any()


def test_hostile_points_hold_every_hostile_word():
    uv = C.hostile_points(2049, 0)
    words = uv.view(np.uint32)
    for bits in C.HOSTILE_BITS:
        assert (words == bits).sum() >= 10, hex(bits)
    assert np.isnan(uv).any() and np.isposinf(uv).any() and np.isneginf(uv).any() and (uv == np.float32(1e30)).any()
    t = C.state(2049, 0)
    st = C.outcome(t, "random", 0)
    hostile = ~np.isfinite(uv).all(axis=1)
    assert (hostile & (t.ids >= 0) & (st == R.TRACKED)).any() and (hostile & (t.ids >= 0) & (st != R.TRACKED)).any()
    t.retire(uv, st)
    assert np.array_equal(t.points.view(np.uint32)[t.ids >= 0], words[t.ids >= 0])  # carried bit for bit


def test_fill_image_spans_more_than_three_rank_tiles():
    survivors = C.fill_survivors()
    S = len(survivors)
    assert S == S_RECORDED and S >= 3 * C.RANK_TILE + 1 and S % C.RANK_TILE != 0
    assert R.survivor_bound(C.HEIGHT, C.WIDTH, C.FILL_MIN_DISTANCE) <= C.MAX_SLOTS
    masked = None
    for n_free in (0, 300, 2048 - C.FILL_MASKING):
        t, uv, st = C.fill_state(2048, n_free, 0)
        free = t.retire(uv, st)
        assert len(free) == n_free and (t.ids[free] < 0).all()
        points, mask = t.occupied()
        got = R.masked_survivors(C.fill_image(), C.FILL_MIN_DISTANCE, C.FILL_MIN_RESPONSE, points, mask)
        assert masked is None or np.array_equal(got, masked)  # the corner slots block nothing: the count does not depend on n_free
        masked = got
    assert len(masked) == S_MASKED_RECORDED and len(masked) % C.RANK_TILE != 0
    gone = {tuple(p) for p in survivors[:2 * C.FILL_MASKING:2]}
    assert not gone & {tuple(p) for p in masked} and {tuple(p) for p in survivors[1:2 * C.FILL_MASKING:2]} <= {tuple(p) for p in masked} | gone
    counts = C.fill_free_counts(2048, len(masked))
    assert counts == [0, 1, 255, 256, 257, len(masked) - 1, len(masked), len(masked) + 3] and counts[-1] <= 2048 - C.FILL_MASKING
