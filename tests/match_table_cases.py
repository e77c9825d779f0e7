"""The hand-written scenarios and the random frames the CPU and GPU tests of the landmark table share: TEST
INFRASTRUCTURE.  A scenario is a table before the call and a matcher's output written by hand; what must come out is written by hand too,
in tests/test_match_table_ref_cpu.py."""
import numpy as np

from tests import match_table_ref as R

T, L, NT, OUT = R.TRACKED, R.LARGE_RESIDUAL, R.NOT_TRACKED, R.OUTSIDE


def cur_rows(k, d=3, base=100.0):
    """Current rows whose values say which row they are: uv (base + j, base + j + 0.5), descriptor all base + j."""
    j = np.arange(k, dtype=np.float32)
    return np.stack([base + j, base + j + 0.5], 1).astype(np.float32), np.repeat((base + j)[:, None], d, 1).astype(np.float32)


def seeded(n, d, live, next_id=None, lost=None):
    """A table whose slots in ``live`` hold ids 10 + s, points (s, s + 0.25), descriptor s everywhere, age 3."""
    t = R.Table(n, d, next_id=10 + n if next_id is None else next_id)
    for s in live:
        t.ids[s], t.points[s], t.prev_points[s], t.descriptors[s] = 10 + s, (s, s + 0.25), (s - 1, s), s
        t.status[s], t.age[s] = T, 3
        t.lost[s] = 0 if lost is None else lost[s]
    t.n_live[0] = len(list(live))
    return t


def scenario(name):
    """(table before, match_index, match_status, K, cur_count, q_count override or None, max_lost) of a hand-written case."""
    i32, u8 = (lambda v: np.array(v, np.int32)), (lambda v: np.array(v, np.uint8))
    if name == "empty table":
        return seeded(4, 3, []), i32([-1] * 4), u8([L] * 4), 3, None, None, 0
    if name == "all hit":
        return seeded(3, 3, [0, 1, 2]), i32([2, 0, 1]), u8([T, T, T]), 3, None, None, 0
    if name == "all miss, max_lost 0":
        return seeded(3, 3, [0, 1, 2]), i32([-1, -1, -1]), u8([L, L, L]), 2, None, None, 0
    if name == "all miss, max_lost 2":
        return seeded(3, 3, [0, 1, 2], lost={0: 0, 1: 1, 2: 2}), i32([-1, -1, -1]), u8([L, L, L]), 2, None, None, 2
    if name == "two rows name one j":
        # rows 0 and 2 name j = 1, row 0 not TRACKED: row 2 is the hit although it is the higher row; rows 1 and 3 both TRACKED name j = 0: row 1 wins
        return seeded(5, 3, [0, 1, 2, 3]), i32([1, 0, 1, 0, -1]), u8([L, T, T, T, L]), 3, None, None, 0
    if name == "rejected match is not admitted":
        # row 0 names j = 0 but the filter rejected it: slot 0 misses (and retires at max_lost 0), j = 0 is claimed: only j = 1 is admitted
        return seeded(3, 3, [0]), i32([0, -1, -1]), u8([L, L, L]), 2, None, None, 0
    if name == "more unclaimed than empty":
        return seeded(3, 3, [1]), i32([4, -1, -1]), u8([T, L, L]), 6, None, None, 0
    if name == "counts above their arrays":
        return seeded(3, 3, [0, 2]), i32([1, 0, 2]), u8([T, T, T]), 3, 99, 99, 0
    if name == "negative counts":
        return seeded(3, 3, [0, 2]), i32([1, 0, 2]), u8([T, T, T]), 3, -5, -7, 0
    if name == "cur_count below a named row":
        # nk = 1: row 0 names j = 1 >= nk, which is no naming: a miss; row 1 names j = 0
        return seeded(3, 3, [0, 2]), i32([1, 0, -1]), u8([T, T, L]), 3, 1, None, 1
    raise KeyError(name)


SCENARIOS = ("empty table", "all hit", "all miss, max_lost 0", "all miss, max_lost 2", "two rows name one j", "rejected match is not admitted",
             "more unclaimed than empty", "counts above their arrays", "negative counts", "cur_count below a named row")


def run(name, mutant=None):
    table, index, status, k, cur_count, q_count, max_lost = scenario(name)
    _, _, q_slot, nq = table.query()
    uv, desc = cur_rows(k, table.dim)
    cur_slot = table.update(q_slot, nq[0] if q_count is None else q_count, index, status, uv, desc, cur_count, max_lost, mutant=mutant)
    return table, cur_slot


def random_frame(rng, table, k, hit_rate=0.6):
    """A frame's matcher output over a table: some rows name rows of the current set (with collisions), some are rejected."""
    _, _, q_slot, nq = table.query()
    index = np.where(rng.random(table.n) < hit_rate, rng.integers(0, k, table.n), -1).astype(np.int32)
    status = np.where((index >= 0) & (rng.random(table.n) < 0.8), T, L).astype(np.uint8)
    uv = rng.random((k, 2)).astype(np.float32) * 100
    desc = rng.standard_normal((k, table.dim)).astype(np.float32)
    return q_slot, nq, index, status, uv, desc
