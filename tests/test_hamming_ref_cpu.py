"""tests/hamming_ref.py on the CPU: the numpy restatement of the Hamming matcher against the C oracle (oracle/oracle_matcher.c), two
texts written apart from the same header, over the width-and-shape sweep that tests/test_matcher_widths_gpu.py runs on the device.

  * exact equality of the indices on every sweep case: ForceMatch and NearbyMatch, thresholds at, just under and just over the planted
    distance, 0, 60 and 3e9, stale indices kept, duplicates, all-zero rows, NaN coordinates (the case: hamming_ref.sweep_case);
  * every mutant of hamming_ref.Flags differs from the unmutated restatement on at least one sweep case: the criterion "equal on the
    sweep" sees each of those misreadings;
  * select(), the whole-array form of the running best, equals the pair-by-pair loops of the header;
  * the return conventions for empty inputs and size mismatches;
  * pack_brief / unpack_brief round-trip at every swept width with the tail bits of the last word zero (both pad paths and the kernels
    count whole words);
  * the plans (csrc/match_plan.cpp, through host/build/match_plan_cli) of what the device tests run reach every form, every
    instantiated width and every pad."""
import dataclasses
import functools

import numpy as np
import pytest

from tests import hamming_ref as H
from tests.test_match_plan_cpu import plan

SWEEP = H.sweep_params()
COL, ROW = H.SWEEP_WINDOW


@functools.lru_cache(maxsize=None)
def sweep_case(n_bits, n_ref, n_cur):
    c = H.sweep_case(n_bits, n_ref, n_cur)
    return c, H.distances(c.ref, c.cur)


def test_sweep_is_the_one_the_issue_sets():
    assert len(SWEEP) == 13 * 3 + 5 * 2
    assert {b for b, _, _ in SWEEP} == set(H.SWEEP_BITS) and {(r, c) for _, r, c in SWEEP} == set(H.SWEEP_SHAPES)
    assert all((r, c) != (513, 1001) for b, r, c in SWEEP if b > 512)


@pytest.mark.parametrize("n_bits,n_ref,n_cur", SWEEP)
def test_equals_the_oracle_on_the_sweep(oracle, n_bits, n_ref, n_cur):
    c, D = sweep_case(n_bits, n_ref, n_cur)
    H.assert_case_is_telling(c, D)
    for thr in c.thresholds + (c.flips - 0.5,):
        for stale in (c.stale, None, c.stale[:5]):
            ok_r, f_r = H.force_match(c.ref, c.cur, thr, stale, D=D)
            ok_o, f_o = oracle.force_match(c.ref, c.cur, thr, stale)
            assert ok_r is True and ok_o is True and np.array_equal(f_r, f_o), (thr, "force")
            with np.errstate(invalid="ignore"):
                ok_r, n_r = H.nearby_match(c.ref, c.cur, c.pred_uv, c.cur_uv, thr, COL, ROW, stale, D=D)
                ok_o, n_o = oracle.nearby_match(c.ref, c.cur, c.pred_uv, c.cur_uv, thr, COL, ROW, stale)
            assert ok_r is True and ok_o is True and np.array_equal(n_r, n_o), (thr, "nearby")
    ok_r, z_r = H.nearby_match(c.ref, c.cur, c.pred_uv, c.cur_uv, 60.0, 0, 0, c.stale, D=D)  # a window of zero: equal coordinates only
    ok_o, z_o = oracle.nearby_match(c.ref, c.cur, c.pred_uv, c.cur_uv, 60.0, 0, 0, c.stale)
    assert np.array_equal(z_r, z_o)


MUTANTS = [f.name for f in dataclasses.fields(H.Flags)]


def test_mutant_list_is_the_one_the_issue_sets():
    assert sorted(MUTANTS) == sorted(["le_threshold", "highest_j_on_ties", "window_ge", "nan_fails_window", "always_reset", "padded_count"])


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_differs_on_a_sweep_case(mutant):
    """Without this, equality with hamming_ref on the sweep — the criterion the device tests use — would not see the misreading."""
    flags = H.Flags(**{mutant: True})
    for n_bits, n_ref, n_cur in SWEEP:
        c, D = sweep_case(n_bits, n_ref, n_cur)
        Dm = H.distances(c.ref, c.cur, flags) if mutant == "padded_count" else D
        for thr in c.thresholds:
            _, good = H.force_match(c.ref, c.cur, thr, c.stale, D=D)
            _, bad = H.force_match(c.ref, c.cur, thr, c.stale, flags, D=Dm)
            if not np.array_equal(good, bad):
                return
            with np.errstate(invalid="ignore"):
                _, good = H.nearby_match(c.ref, c.cur, c.pred_uv, c.cur_uv, thr, COL, ROW, c.stale, D=D)
                _, bad = H.nearby_match(c.ref, c.cur, c.pred_uv, c.cur_uv, thr, COL, ROW, c.stale, flags, D=Dm)
            if not np.array_equal(good, bad):
                return
    pytest.fail(f"no sweep case tells {mutant} from the rule")


@pytest.mark.parametrize("mutant,n_bits", [("le_threshold", 257), ("highest_j_on_ties", 480), ("window_ge", 96), ("nan_fails_window", 544),
                                           ("always_reset", 1), ("padded_count", 300)])
def test_each_mutant_is_seen_where_the_case_plants_it(mutant, n_bits):
    """The planted features do what they are there for, one by one, at a width of each kind."""
    flags = H.Flags(**{mutant: True})
    c, D = sweep_case(n_bits, 130, 95)
    Dm = H.distances(c.ref, c.cur, flags)
    thr = {"le_threshold": float(c.flips)}.get(mutant, c.flips + 0.5)
    with np.errstate(invalid="ignore"):
        _, good = H.nearby_match(c.ref, c.cur, c.pred_uv, c.cur_uv, thr, COL, ROW, c.stale, D=D)
        _, bad = H.nearby_match(c.ref, c.cur, c.pred_uv, c.cur_uv, thr, COL, ROW, c.stale, flags, D=Dm)
    differ = set(np.flatnonzero(good != bad).tolist())
    if mutant == "window_ge":
        assert c.partner[4] in differ and good[c.partner[4]] == 4   # the candidate exactly on the window's edge
    if mutant == "nan_fails_window":
        assert {c.partner[6], c.partner[9]} <= differ and good[c.partner[6]] == 6 and good[c.partner[9]] == 9
    if mutant == "always_reset":
        assert (good[sorted(differ)] >= 7000).all() and (bad[sorted(differ)] == -1).all()
    _, good = H.force_match(c.ref, c.cur, thr, c.stale, D=D)
    _, bad = H.force_match(c.ref, c.cur, thr, c.stale, flags, D=Dm)
    assert differ or (good != bad).any(), mutant
    if mutant == "highest_j_on_ties":
        assert good[c.partner[3]] == 3 and bad[c.partner[3]] == c.cur.shape[0] // 2
    if mutant == "le_threshold":
        rows = np.unique(c.partner[c.partner >= 0])  # every planted pair sits AT the threshold
        assert (good[rows] == c.stale[rows]).all() and (bad[rows] < 7000).all() and good[7] == 11


@pytest.mark.parametrize("n_bits", [1, 33, 96])
def test_select_equals_the_loops_as_written(n_bits):
    c, D = sweep_case(n_bits, 65, 33)
    for thr in c.thresholds:
        for stale in (c.stale, None):
            assert np.array_equal(H.force_match(c.ref, c.cur, thr, stale, D=D)[1], H.scan_literal(c.ref, c.cur, thr, stale)), thr
            with np.errstate(invalid="ignore"):
                got = H.nearby_match(c.ref, c.cur, c.pred_uv, c.cur_uv, thr, COL, ROW, stale, D=D)[1]
            assert np.array_equal(got, H.scan_literal(c.ref, c.cur, thr, stale, c.pred_uv, c.cur_uv, COL, ROW)), thr


def test_distances_are_compute_distance_of_each_pair():
    for n_bits in (1, 33, 300, 2048):
        c, D = sweep_case(n_bits, 65, 33)
        assert D.dtype == np.float32 and D.shape == (65, 33)
        rs = np.random.RandomState(n_bits)
        for i, j in zip(rs.randint(0, 65, 40), rs.randint(0, 33, 40)):
            assert D[i, j] == H.distance_pair(c.ref[i], c.cur[j])
        assert D[7, 11] == 0 and D[c.partner[3], 3] == c.flips == D[c.partner[3], 33 // 2]
    big = H.distances(np.ones((H.ROW_BLOCK + 3, 40), np.uint8), np.zeros((2, 40), np.uint8))  # more than one row block
    assert (big == 40).all()
    assert H.distance_pair(np.zeros(0, np.uint8), np.zeros(0, np.uint8)) == np.float32(2 ** 31)


def test_empty_descriptors_give_kmaxint32(oracle):
    """n_bits == 0: ComputeDistance is kMaxInt32 for every pair (test_descriptor_matcher_brief.cpp:34-36): candidate 0 under a threshold
    above 2^31, nothing below it."""
    ref, cur = np.zeros((4, 0), np.uint8), np.zeros((6, 0), np.uint8)
    uv_r, uv_c = np.zeros((4, 2), np.float32), np.zeros((6, 2), np.float32)
    stale = np.arange(4, dtype=np.int32) + 7000
    assert (H.distances(ref, cur) == np.float32(2 ** 31)).all()
    for thr, want in ((60.0, stale), (2147483648.0, stale), (3e9, np.zeros(4, np.int32))):
        ok, f = H.force_match(ref, cur, thr, stale)
        assert ok and np.array_equal(f, want) and np.array_equal(f, oracle.force_match(ref, cur, thr, stale)[1]), thr
        ok, n = H.nearby_match(ref, cur, uv_r, uv_c, thr, 40, 40, stale)
        assert ok and np.array_equal(n, want) and np.array_equal(n, oracle.nearby_match(ref, cur, uv_r, uv_c, thr, 40, 40, stale)[1]), thr


def test_return_conventions(oracle):
    """descriptor_matcher.h:58-62 and :94-100."""
    c, _ = sweep_case(33, 65, 33)
    held = np.arange(65, dtype=np.int32) + 7000
    for stale in (None, held, held[:9]):
        # no candidates: false, index_pairs untouched (the size check of :60 comes after)
        ok, idx = H.force_match(c.ref, c.cur[:0], 60.0, stale)
        ok_o, idx_o = oracle.force_match(c.ref, c.cur[:0], 60.0, stale)
        assert ok is False and ok_o is False and np.array_equal(idx, idx_o) and np.array_equal(idx, np.zeros(0, np.int32) if stale is None else stale)
        for pred, cuv, cur in ((c.pred_uv, c.cur_uv[:0], c.cur[:0]), (c.pred_uv[:64], c.cur_uv, c.cur), (c.pred_uv, c.cur_uv[:32], c.cur)):
            ok, idx = H.nearby_match(c.ref, cur, pred, cuv, 60.0, COL, ROW, stale)
            ok_o, idx_o = oracle.nearby_match(c.ref, cur, pred, cuv, 60.0, COL, ROW, stale)
            assert ok is False and ok_o is False and np.array_equal(idx, idx_o) and np.array_equal(idx, np.zeros(0, np.int32) if stale is None else stale)
        # no reference rows: true, an empty list
        ok, idx = H.force_match(c.ref[:0], c.cur, 60.0, stale)
        ok_o, idx_o = oracle.force_match(c.ref[:0], c.cur, 60.0, stale)
        assert ok is True and ok_o is True and idx.size == 0 and idx_o.size == 0
    # a list of another size is reset, one of the same size is kept where nothing matches
    assert (H.force_match(c.ref, c.cur, 0.0, held[:9])[1] == -1).all() and np.array_equal(H.force_match(c.ref, c.cur, 0.0, held)[1], held)


@pytest.mark.parametrize("n_bits", H.SWEEP_BITS)
def test_pack_round_trip_and_zero_tail(ftk, n_bits):
    c, _ = sweep_case(n_bits, 65, 33)
    bits = c.ref.copy()
    bits[1] = 1  # a row of ones: its tail would show
    words = ftk.pack_brief(bits)
    n_words = (n_bits + 31) // 32
    assert words.dtype == np.uint32 and words.shape == (65, n_words)
    assert np.array_equal(ftk.unpack_brief(words, n_bits), bits)
    tail = n_bits % 32
    if tail:
        assert not (words[:, -1] >> np.uint32(tail)).any()
        assert words[1, -1] == (1 << tail) - 1
    # bit k of the descriptor is bit k % 32 of word k // 32
    k = n_bits - 1
    assert np.array_equal((words[:, k // 32] >> np.uint32(k % 32)) & 1, bits[:, k])


# ---- what the device tests reach ----

def device_test_plans():
    """(what, plan) of every Hamming call of tests/test_matcher_widths_gpu.py: (n_bits, shape) x FTK_MATCH_SMALL x FTK_MATCH_KERNEL x
    ForceMatch / NearbyMatch.  n_words is the caller's width: `pad` and `dev_words` say what the entry pads it to (the host entry
    during its gather, the device entry with pad_descriptors)."""
    from tests import test_matcher_widths_gpu as G
    cases, what = [], []
    for (n_bits, n_ref, n_cur), small, kernel, nearby in G.hamming_calls():
        d = dict(n_ref=n_ref, n_cur=n_cur, n_words=max(1, (n_bits + 31) // 32), n_bits=n_bits, nearby=nearby)
        if small is not None:
            d["small"] = small
        if kernel is not None:
            d["kernel"] = kernel
        cases.append(d)
        what.append((n_bits, n_ref, n_cur, small, kernel, nearby))
    return list(zip(what, plan("hamming", cases)))


def test_device_tests_reach_every_form_width_and_pad():
    rows = device_test_plans()
    reached = {(p["form"], p["dev_words"]) for _, p in rows}
    assert {("popcount", w) for w in (1, 2, 4, 8, 16)} <= reached
    assert {("matrix_cores", 8), ("matrix_cores", 16)} <= reached
    assert {f for f, _ in reached} == {"small", "popcount", "matrix_cores", "plain", "generic"}
    assert {("small", w) for w in (1, 2, 4, 8, 16)} <= reached
    pads = {(w[0] + 31) // 32: p["dev_words"] for w, p in rows if p["pad"]}
    assert pads[3] == 4 and all(pads[w] == 8 for w in (5, 7)) and all(pads[w] == 16 for w in (9, 10, 15)), pads
    assert any(p["form"] == "generic" and p["n_boxes"] > 0 and p["box_grid"][0] == 0 for _, p in rows)  # boxes reserved, not launched
    assert any(p["form"] == "matrix_cores" and p["cur_per_block"] == 1024 * 32 for _, p in rows)       # a 1024-tile split
