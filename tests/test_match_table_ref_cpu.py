"""The landmark table's restatement (tests/match_table_ref.py) against answers written by hand from the contract (include/ftk.h,
DESIGN.md 5.28), its invariants over random sequences, the mutants these checks catch, and the synthetic video sequence through the
restatements alone (tests/match_video_cases.py).  The scenarios are tests/match_table_cases.py's, shared with tests/test_match_table_gpu.py."""
import numpy as np
import pytest

from tests import match_table_ref as R
from tests.match_table_cases import L, NT, OUT, SCENARIOS, T, random_frame, run, seeded


def test_query_lists_the_live_slots_in_order():
    t = seeded(5, 3, [1, 4])
    q_uv, q_desc, q_slot, nq = t.query()
    assert nq[0] == 2 and q_slot.tolist() == [1, 4, -1, -1, -1]
    assert q_uv.tolist() == [[1, 1.25], [4, 4.25], [0, 0], [0, 0], [0, 0]] and q_desc[:, 0].tolist() == [1, 4, 0, 0, 0]
    assert not np.signbit(q_uv[2:]).any() and not np.signbit(q_desc[2:]).any()
    assert R.Table(3, 2).query()[3][0] == 0 and seeded(2, 1, [0, 1]).query()[2].tolist() == [0, 1]


def test_known_answers():
    t, cs = run("empty table")
    assert t.ids.tolist() == [0 + 14, 1 + 14, 2 + 14, -1] and cs.tolist() == [0, 1, 2] and t.next_id[0] == 17 and t.n_live[0] == 3
    assert t.points[:3].tolist() == [[100, 100.5], [101, 101.5], [102, 102.5]] and (t.points[:3] == t.prev_points[:3]).all()
    assert t.status.tolist() == [NT, NT, NT, OUT] and t.age.tolist() == [0] * 4 and t.descriptors[:, 0].tolist() == [100, 101, 102, 0]

    t, cs = run("all hit")
    assert t.ids.tolist() == [10, 11, 12] and cs.tolist() == [1, 2, 0] and t.next_id[0] == 13 and t.n_live[0] == 3
    assert t.points[:, 0].tolist() == [102, 100, 101] and t.prev_points.tolist() == [[0, 0.25], [1, 1.25], [2, 2.25]]
    assert t.descriptors[:, 2].tolist() == [102, 100, 101] and t.age.tolist() == [4, 4, 4] and t.lost.tolist() == [0, 0, 0] and t.status.tolist() == [T] * 3

    t, cs = run("all miss, max_lost 0")  # every slot retires and is free for the two current rows at once
    assert t.ids.tolist() == [13, 14, -1] and cs.tolist() == [0, 1] and t.next_id[0] == 15 and t.n_live[0] == 2
    assert t.status.tolist() == [NT, NT, L] and t.lost.tolist() == [0, 0, 1] and t.points[2].tolist() == [2, 2.25] and t.age.tolist() == [0, 0, 3]

    t, cs = run("all miss, max_lost 2")  # lost 0, 1, 2 -> 1, 2, 3: only the last exceeds 2
    assert t.ids.tolist() == [10, 11, 13] and t.lost.tolist() == [1, 2, 0] and t.status.tolist() == [L, L, NT] and cs.tolist() == [2, -1]
    assert t.next_id[0] == 14 and t.n_live[0] == 3 and t.points[:2].tolist() == [[0, 0.25], [1, 1.25]] and t.age.tolist() == [3, 3, 0]

    t, cs = run("two rows name one j")
    assert t.status.tolist() == [NT, T, T, L, OUT] and cs.tolist() == [1, 2, 0]  # j = 2 is unclaimed: slots 0 and 3 retire, it takes slot 0
    assert t.ids.tolist() == [15, 11, 12, -1, -1] and t.next_id[0] == 16 and t.n_live[0] == 3
    assert t.points[:3, 0].tolist() == [102, 100, 101] and t.age.tolist() == [0, 4, 4, 3, 0]

    t, cs = run("rejected match is not admitted")
    assert cs.tolist() == [-1, 0] and t.ids.tolist() == [13, -1, -1] and t.points[0].tolist() == [101, 101.5] and t.next_id[0] == 14 and t.n_live[0] == 1

    t, cs = run("more unclaimed than empty")  # j = 4 is the hit; j = 0, 1 go to slots 0, 2; j = 2, 3, 5 find no slot
    assert cs.tolist() == [0, 2, -1, -1, 1, -1] and t.ids.tolist() == [13, 11, 14] and t.next_id[0] == 15 and t.n_live[0] == 3

    for name in ("counts above their arrays", "negative counts"):
        t, cs = run(name)
        if name.startswith("counts above"):  # nq = 3 but row 2's slot is -1: rows 0, 1 hit j = 1, 0; j = 2 is named by row 2, so claimed
            assert cs.tolist() == [2, 0, -1] and t.ids.tolist() == [10, -1, 12] and t.next_id[0] == 13
        else:  # nq = 0 and nk = 0: nothing happens at all
            assert cs.tolist() == [-1, -1, -1] and t.ids.tolist() == [10, -1, 12] and t.lost.tolist() == [0, 0, 0] and t.next_id[0] == 13
            assert t.status.tolist() == [T, OUT, T] and t.n_live[0] == 2

    t, cs = run("cur_count below a named row")
    assert cs.tolist() == [2, -1, -1] and t.ids.tolist() == [10, -1, 12] and t.lost.tolist() == [1, 0, 0] and t.status.tolist() == [L, OUT, T]
    assert t.next_id[0] == 13 and t.n_live[0] == 2


@pytest.mark.parametrize("seed", range(6))
def test_invariants_over_random_sequences(seed):
    rng = np.random.default_rng(seed)
    n, d, max_lost = int(rng.integers(1, 40)), 3, int(rng.integers(0, 3))
    table = R.Table(n, d)
    for _ in range(12):
        k = int(rng.integers(1, 30))
        before, next_before = table.ids.copy(), int(table.next_id[0])
        q_slot, nq, index, status, uv, desc = random_frame(rng, table, k)
        cur_slot = table.update(q_slot, nq[0], index, status, uv, desc, int(rng.integers(0, k + 2)), max_lost)
        live = table.ids[table.ids >= 0]
        assert len(set(live.tolist())) == len(live) and table.n_live[0] == len(live)
        new = [(j, int(table.ids[s])) for j, s in enumerate(cur_slot) if s >= 0 and table.ids[s] >= next_before]
        assert [i for _, i in new] == list(range(next_before, int(table.next_id[0])))  # new ids are next_id .., ascending in j
        for s in range(n):  # a slot index never changes under a live id
            if before[s] >= 0 and table.ids[s] >= 0 and table.ids[s] < next_before:
                assert table.ids[s] == before[s]
        assert all(int(i) not in before.tolist() or int(np.where(before == i)[0][0]) == int(np.where(table.ids == i)[0][0]) for i in live)


def _all_scenarios(mutant):
    out = []
    for name in SCENARIOS:
        t, cs = run(name, mutant)
        out.append([v.copy() for v in t.tensors().values()] + [cs])
    return out


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_each_mutant_is_caught(mutant):
    good, bad = _all_scenarios(None), _all_scenarios(mutant)
    same = all(np.array_equal(a, b) for g, m in zip(good, bad) for a, b in zip(g, m))
    assert not same, f"the mutant {mutant} changes nothing these cases see"


def test_the_video_sequence_through_the_restatements_is_the_hand_written_history():
    from tests import match_video_cases as V
    history, frames = V.expected_ids(), V.compose()
    for f, (tensors, cur_slot) in enumerate(frames):
        seen = V.ids_by_landmark(f, tensors, cur_slot)
        assert seen == {l: history[f][l] for l in seen}, f
        assert sorted(int(i) for i in tensors["ids"] if i >= 0) == sorted(history[f].values()), f
    last = history[-1]
    assert all(last[l] == history[0][l] for l in V.SHORT) and all(last[l] >= 44 for l in V.LONG)  # kept / returned under new ids
    assert all(l not in history[4] for l in V.LONG) and all(l in history[3] for l in V.LONG)
    bad = V.compose(mutant="retire_at_max_lost")
    assert any(V.ids_by_landmark(f, *bad[f]) != V.ids_by_landmark(f, *frames[f]) for f in range(V.FRAMES))
