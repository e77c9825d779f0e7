"""What tests/test_sparse_entries_guarded_gpu.py rests on, without a device:

 (i)   the KLT option sets of that file walked through ``klt_plan`` (the host plan program of tests/test_klt_plan_cpu.py): every set runs
       the launch form it names, all four forms are reached, and the feature counts are 1, g, g + 1 and an odd count of a few workgroups
       for the plan's own features per workgroup g.  ``klt_counts`` is where the GPU file takes its counts from;
 (ii)  every matcher, NN, table, Harris, BRIEF and dense shape has the tail it is claimed to have, against the plan programs and the tile
       constants;
 (iii) every spec list passes the argument checks of its entry: the same arenas built on CPU tensors, the entries run up to their native
       call over a recording stand-in of the library, and a written payload one element off is refused before it.
"""
import functools
import os
import re
import types

import numpy as np
import pytest

from tests import args_walk as A
from tests import guarded as G
from tests import test_klt_plan_cpu as KP
from tests import test_sparse_entries_guarded_gpu as E
from tests import track_table_ref as TR

torch = pytest.importorskip("torch")

import feature_tracker_amd as F  # noqa: E402
from feature_tracker_amd import _native as N  # noqa: E402
from feature_tracker_amd import device as D  # noqa: E402

MODELS = {"basic": KP.BASIC, "affine": KP.AFFINE, "lssd": KP.LSSD}
METHODS = {"inverse": KP.INVERSE, "direct": KP.DIRECT, "fast": KP.FAST}
FORMS = {"pipelined", "one_wave_fast", "generic", "generic_spill"}


# ---- (i) the KLT forms and counts --------------------------------------------------------------------------------------------------------------

def klt_plans(k, counts):
    """The plan of KLT_SETS[k] at every feature count of ``counts``, as the library plans the call: exact reduction mode, the pinned tail class."""
    _, model, method, lum, half, tail, (w, h, _), _ = E.KLT_SETS[k]
    return KP.plan([dict(model=MODELS[model], method=METHODS[method], half=(half, half), n=n, max_extent=max(w, h), lum=int(lum), long_tail=tail)
                    for n in counts])


@functools.lru_cache(maxsize=None)
def klt_counts(k):
    """(g, the sorted counts {1, g, g + 1, an odd count of more than three workgroups whose last one is partial})."""
    g = klt_plans(k, [1])[0]["features_per_group"]
    several = 3 * g + (g - 1 if g > 1 else 2)
    return g, tuple(sorted({1, g, g + 1, several}))


def test_every_klt_set_runs_the_form_it_names_at_the_counts_of_its_plan():
    seen, groups = set(), set()
    for k, (name, model, method, lum, half, tail, scene, form) in enumerate(E.KLT_SETS):
        g, counts = klt_counts(k)
        plans = klt_plans(k, counts)
        for n, p in zip(counts, plans):
            what = (name, n, p)
            assert p["rc"] == 0 and p["kernel"] == 1 and p["form"] == form, what
            assert p["features_per_group"] == g and p["grid"] == -(-n // g) and p["long_tail"] == tail and p["tree"] == 0, what
        several = max(counts)
        assert {1, g, g + 1} <= set(counts) and several % 2 == 1 and several > 3 * g and (g == 1 or several % g != 0) and (g <= 2 or several % g != 1), (name, g, counts)
        assert g == 1 or (g + 1) % g == 1  # the last workgroup of g + 1 features holds one
        assert E.KLT_OPTION_CAP > several and all(E.klt_cap(n) == n - 1 for n in counts if n > 1)
        assert len(E.klt_features(k)) >= several
        seen.add((form, model, method, bool(lum), plans[0]["lssd_chunked"], plans[0]["k_lum"], plans[0]["solo"]))
        groups.add((form, g))
        runs = E.klt_runs(k)
        assert {(n, r) for n in counts for r in E.KLT_RUNS_AT_EVERY_COUNT} <= set(runs) and {r for _, r in runs} == set(E.KLT_RUNS)
    assert {s[0] for s in seen} == FORMS  # zero forms missing
    assert {("pipelined", "basic", "inverse")} == {s[:3] for s in seen if s[0] == "pipelined"}
    assert {s[6] for s in seen if s[0] == "pipelined"} == {0, 1}  # a feature on several waves, and the solo form of several features per workgroup
    assert {s[1:3] for s in seen if s[0] == "one_wave_fast"} == {("basic", "fast"), ("affine", "fast")}
    generic = {s[1:4] for s in seen if s[0] == "generic"}
    assert {m for m, _, _ in generic} == set(MODELS) and all(any(m == model and method != "fast" for m, method, _ in generic) for model in MODELS)
    assert {("lssd", "fast", False), ("lssd", "fast", True), ("lssd", "inverse", True)} <= generic
    assert any(s[4] == 1 and s[5] == 0 for s in seen) and any(s[5] == 1 for s in seen)  # the chunked LSSD level without and with luminance
    assert any(g > 1 for f, g in groups if f == "pipelined") and any(g > 1 for f, g in groups if f == "one_wave_fast") and any(g > 1 for f, g in groups if f == "generic")
    spill = [s for s in E.KLT_SETS if s[7] == "generic_spill"]
    assert spill and all(s[4] == 30 and s[6] == (640, 480, 2) for s in spill)  # the half patch and scene of tests/test_klt_gpu.py's large-patch case
    source = open(os.path.join(A.ROOT, "tests", "test_klt_gpu.py")).read()
    assert '("affine", "inverse", 30)' in source and "scenes.scene(640, 480, 2)" in source
    # some features arrive above tracked at the largest count; the single feature of the last workgroup of g + 1 is not one of them
    for k in range(len(E.KLT_SETS)):
        g, counts = klt_counts(k)
        assert (E.klt_case(k, max(counts), False)[0]["status_in"] > 1).any() and E.klt_case(k, g + 1, False)[0]["status_in"][g] <= 1


# ---- (ii) the shapes reach their tails -----------------------------------------------------------------------------------------------------------

def _match_plans(lines):
    out = A.run_plan_tool(A.plan_cli("match_plan_cli"), lines, timeout=120)
    return [{k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in p.items()} for p in out]


def test_the_matcher_shapes_have_a_tail_on_both_axes():
    (n_ref, n_cur), one = E.MATCH_COUNTS
    assert one == (1, 1) and set(E.HAMMING_BITS) == {256, 96, 32} and E.COSINE_DIMS == (256, 100)
    for n_bits in E.HAMMING_BITS:
        words = (n_bits + 31) // 32
        for nearby in (0, 1):
            for keys in (0, 1):
                p, = _match_plans([("hamming", n_ref, n_cur, words, n_bits, nearby, keys, "-", "-")])
                blocks = int(p["scan_grid"].split("x")[0])
                per_block = -(-n_ref // blocks)
                assert blocks >= 2 and n_ref % per_block, (n_bits, p)              # the last workgroup holds fewer reference rows
                assert n_cur > p["cur_per_block"] and n_cur % p["cur_per_block"], (n_bits, p)  # a partial last tile of candidates behind whole ones
                assert p["matrix_cores"] == int(n_bits == 256) and p["dev_words"] == {8: 8, 3: 4, 1: 1}[words], (n_bits, p)
    for dim in E.COSINE_DIMS:
        for nearby in (0, 1):
            forms = set()
            for small in ("-", 0):  # the default and FTK_COSINE_SMALL=0
                p, = _match_plans([("cosine", n_ref, n_cur, dim, nearby, 1, small, "-", "-")])
                forms.add(p["form"])
                assert p["n_ref_pad"] > n_ref and p["n_cur_pad"] > n_cur and n_cur > p["n_cur_pad"] - n_cur, (dim, p)  # both axes padded: a partial tile on each
            assert "register_stationary" in forms, (dim, forms)
    assert any(dim % 16 for dim in E.COSINE_DIMS)  # a row that is no whole number of 16-float packets
    # the spoiled reference rows keep their stale entry, the others find a pair: index_pairs is written and kept in one call
    for n_bits in E.HAMMING_BITS:
        for nearby in (False, True):
            _, stale, want, _ = E.hamming_case(n_bits, n_ref, n_cur, nearby)
            assert (want == stale)[E._unmatched(n_ref)].sum() >= 3 and (want < E.STALE).sum() > 20, (n_bits, nearby)
    for dim in E.COSINE_DIMS:
        for nearby in (False, True):
            _, stale, want = E.cosine_case(dim, n_ref, n_cur, nearby)
            assert (want == stale)[E._unmatched(n_ref)].sum() >= 3 and (want < E.STALE).sum() > 20, (dim, nearby)


def test_the_nn_shapes_have_a_tail_on_both_axes():
    plans = _match_plans([("nn", 1, n_ref, n_cur, n_cur, 0, 1) for n_ref, n_cur in E.NN_SCORE_SHAPES])
    assert all(p["ok"] == 1 for p in plans) and E.NN_SCORE_SHAPES[0] == (1, 1)
    for (n_ref, n_cur), p in list(zip(E.NN_SCORE_SHAPES, plans))[1:]:
        assert n_ref % p["tile_rows"] and p["row_tiles"] >= 2, (n_ref, n_cur, p)
        assert n_cur % p["tile_cols"], (n_ref, n_cur, p)
    assert any(p["col_tiles"] >= 2 for p in plans) and {p["vec4"] for p in plans} == {0, 1}
    for n_ref, n_cur in E.NN_LIST_SHAPES:
        assert n_ref % 64 and n_ref % 256
    assert any(r < 64 for r, _ in E.NN_LIST_SHAPES) and any(64 < r < 256 for r, _ in E.NN_LIST_SHAPES) and any(r > 256 for r, _ in E.NN_LIST_SHAPES)
    assert any(c < 256 for _, c in E.NN_LIST_SHAPES) and any(c > 256 for _, c in E.NN_LIST_SHAPES) and any(r > c for r, c in E.NN_LIST_SHAPES)
    for n_ref, n_cur in E.NN_LIST_SHAPES:
        matches, _, idx, _, _ = E.nn_list_case(n_ref, n_cur)
        assert (matches < 0).any() and (matches[:, 0] >= n_ref).any() and (matches[:, 1] >= n_cur).any() and (idx >= 0).any() and (idx < 0).any()


def test_the_table_shapes_stand_at_the_edges_of_the_plan():
    tile, block = N.FTK_HARRIS_RANK_TILE, N.FTK_TRACK_TABLE_BLOCK
    assert E.TABLE_SIZES == (1, tile - 1, tile, tile + 1, block + 1)
    rows, cols = E.TC.HEIGHT, E.TC.WIDTH
    plans = A.run_plan_tool(A.plan_cli("track_table_plan_cli"), [(rows, cols, E.TC.FILL_MIN_DISTANCE, n, n) for n in E.TABLE_SIZES], timeout=120)
    assert all(p["refused"] == "none" and int(p["rank_tile"]) == tile and int(p["retire_block"]) == block for p in plans)
    assert [int(p["retire_per_thread"]) for p in plans] == [1, 1, 1, 1, 2]  # 1025: two slots per thread, the last owner holds one
    for n in E.TABLE_SIZES:
        names = [c[0] for c in E.retire_cases(n)]
        assert names == list(E.TABLE_PATTERNS) + ["forward-backward"]
        for name, make, uv, status, back_uv, back_status, threshold in E.retire_cases(n):
            before, after = make(), make()
            free = after.retire(uv, status, back_uv, back_status, threshold)
            assert (name != "all_empty" or len(free) == n) and (name != "all_dead" or len(free) == n)
            if name == "random" and n > 1:
                assert 0 < len(free) < n and (before.ids < 0).any()  # slots that are empty before the call, slots it retires, slots that stay
    # the match table: four flags per thread of the one scan workgroup, four rows per workgroup of the movers, waves of 64
    text = open(os.path.join(A.ROOT, "feature_tracker_amd", "csrc", "match_table_plan.h")).read()
    assert int(re.search(r"kMatchTableMoveWaves = (\d+);", text).group(1)) == 4 and N.FTK_MATCH_TABLE_MAX_SLOTS == 4 * block
    shapes = []
    for case in range(len(E.MATCH_TABLE_CASES)):
        make, index, status, uv, desc, cur_count, q_count, max_lost, with_slot = E.match_table_case(case)
        shapes.append((make().n, uv.shape[0], cur_count is not None, with_slot))
        assert make().n % 4 and uv.shape[0] % 4  # a tail on the slot axis and on the current-row axis
    assert (5, 3) in {s[:2] for s in shapes} and any(n > 64 and n % 64 and k > 64 and k % 64 for n, k, _, _ in shapes)
    assert {s[2] for s in shapes} == {False, True} and {s[3] for s in shapes} == {False, True}
    n, k, d = E.MATCH_TABLE_RANDOM
    words = dict((s[0], s[2]) for s in E.match_table_specs(1))["workspace"]
    assert words == (-(-N.match_table_workspace_bytes(n, k, d) // 8),) and 8 * words[0] - 4 * k < 16  # the declared bytes, with no added term


def test_the_harris_brief_and_dense_cases_are_what_they_claim(oracle):
    assert [c[0] for c in E.HARRIS_CASES] == [(23, 23), (64, 48), (333, 251)]
    no_survivor = False
    for size, distance, occupied in E.harris_runs():
        image, points, mask, survivors = E.harris_case(size, distance, occupied)
        S = len(survivors)
        counts = E.harris_max_counts(S)
        assert set(counts) == {c for c in (S - 1, S, S + 3) if c >= 1} and S + 3 in counts
        no_survivor |= S == 0
        assert (occupied == "none") == (points is None)
    assert no_survivor  # count_out = 0 and nothing but zeros in uv_out must be WRITTEN there
    runs = {(size, occupied) for size, _, occupied in E.harris_runs()}
    for size, _ in E.HARRIS_CASES:
        assert (size, "none") in runs and (size, "dense_random") in runs
        assert E.harris_case(size, dict(E.HARRIS_CASES)[size], "dense_random")[2] is not None  # the mask
    assert len(E.harris_case((333, 251), 2, "none")[3]) > 2 * N.FTK_HARRIS_RANK_TILE
    # BRIEF: a partial last word, rows of zeros next to rows with bits, at both half patches
    assert E.BRIEF_BITS == (256, 100, 32) and E.BRIEF_COUNTS == (1, 65) and E.BRIEF_HALVES == (8, 63) and 100 % 32
    for half in E.BRIEF_HALVES:
        for n_bits in E.BRIEF_BITS:
            want = E.brief_want(65, n_bits, half)
            zero = ~want.any(axis=1)
            assert want.shape == (65, (n_bits + 31) // 32) and 4 <= zero.sum() < 10 and E.brief_want(1, n_bits, half).any(), (half, n_bits, zero.sum())
            if n_bits % 32:
                assert not (want[:, -1] >> np.uint32(n_bits % 32)).any() and want[:, -1].any()
    # dense flow: the kernels' tile, from their source
    text = open(os.path.join(A.ROOT, "feature_tracker_amd", "csrc", "dense_flow_kernels.hip")).read()
    tile = int(re.search(r"constexpr int kTile = (\d+);", text).group(1))
    from tests.test_dense_flow_gpu import test_odd_and_tiny_sizes
    own = [tuple(v) for v in next(m for m in test_odd_and_tiny_sizes.pytestmark if m.name == "parametrize").args[1]]
    assert set(E.DENSE_CASES) <= set(own)
    whole = [c for c in own if all((c[0] >> l) > tile and (c[1] >> l) > tile and (c[0] >> l) % tile and (c[1] >> l) % tile for l in range(c[2]))]
    assert whole and min(whole, key=lambda c: c[0] * c[1]) == E.DENSE_CASES[0]  # a partial tile behind whole ones, both axes, every level
    assert E.DENSE_CASES[1] == (4, 5, 1) and all(0 < e < tile for e in E.DENSE_CASES[1][:2])  # one partial tile on both axes, more than one row of it
    for w, h, levels in E.DENSE_CASES:
        shapes = dict((s[0], s[2]) for s in E.dense_specs(w, h, levels))
        assert shapes["flow_r"] == shapes["flow_c"] == shapes["ref0"] == (h, w)


# ---- (iii) the spec lists against the entries' own checks ----------------------------------------------------------------------------------------

class Recorder:
    """Stands where the loaded library stands: every entry is recorded and answers FTK_OK; nothing is launched."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("ftk_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            return 0

        return entry


class Pyramid:
    """What the entries ask of a pyramid: a handle and the levels' shapes, here those of the payloads it was made of."""
    handle = None

    def __init__(self, desc):
        self.desc = desc

    def level_desc(self, i):
        return self.desc[i]

    @classmethod
    def from_device_levels(cls, desc, ctx, keepalive=None):
        return cls(list(desc))


class OnDevice(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` as a CUDA tensor does, for the NN entries, which ask torch's own tensor type inline."""
    is_cuda = property(lambda self: True)


class DeviceViews:
    def __init__(self, arena):
        self.arena = arena

    def __getitem__(self, name):
        return self.arena[name].as_subclass(OnDevice)


@pytest.fixture
def walk(monkeypatch):
    """The entries on CPU tensors: every check of dtype, shape, element count and stride is the real one, only where a tensor lives is not
    asked, and the library is the recorder."""
    recorder = Recorder()
    stream = types.SimpleNamespace(cuda_stream=0)
    fake_torch = types.SimpleNamespace(cuda=types.SimpleNamespace(current_stream=lambda device=None: stream), Tensor=torch.Tensor, float32=torch.float32,
                                       int32=torch.int32, int64=torch.int64, uint8=torch.uint8)
    monkeypatch.setattr(N, "lib", lambda: recorder)
    monkeypatch.setattr(D, "_torch", lambda: fake_torch)
    monkeypatch.setattr(D, "_device_complaint", lambda name, t, device_index: None)
    monkeypatch.setattr(D, "ImagePyramid", Pyramid)
    return types.SimpleNamespace(lib=recorder, ctx=types.SimpleNamespace(handle=None, device_index=None))


def _arena(specs, inputs):
    arena = E.make_arena(specs, inputs, G.ONES, "cpu")
    for name, _, shape, _ in specs:  # (a) and (e): exactly the spec's elements, on a 256-byte boundary
        assert tuple(arena[name].shape) == shape and arena[name].data_ptr() % G.ALIGN == 0 and arena[name].is_contiguous()
    return arena


def _one_off(specs, name):
    """The spec list with payload ``name`` one element shorter in its last dimension (longer where that is 1)."""
    out = []
    for n, dtype, shape, fill in specs:
        if n == name:
            shape = shape[:-1] + (shape[-1] - 1 if shape[-1] > 1 else 2,)
        out.append((n, dtype, shape, fill))
    return out


def _walk_entry(walk, specs, inputs, call, native, written, views=lambda arena: arena):
    """``call(arena)`` passes every check and reaches exactly ``native``; with a written payload one element off it is refused before."""
    names = [s[0] for s in specs]
    assert set(written) <= set(names) and set(inputs) <= set(names), (written, names)
    del walk.lib.calls[:]
    call(views(_arena(specs, inputs)))
    assert walk.lib.calls == native, walk.lib.calls
    for name in written:
        del walk.lib.calls[:]
        with pytest.raises(ValueError, match="must"):
            call(views(E.make_arena(_one_off(specs, name), {k: v for k, v in inputs.items() if k != name}, G.ONES, "cpu")))
        assert walk.lib.calls == [], name
    del walk.lib.calls[:]


def test_klt_and_direct_specs_pass_the_entries_checks(walk):
    for k in range(len(E.KLT_SETS)):
        levels = E.KLT_SETS[k][6][2]
        for n, run in E.klt_runs(k):
            iters, capped, alias, _ = E.KLT_RUNS[run]
            inputs, _ = E.klt_case(k, n, capped)
            written = (["cur_uv_in", "status_in"] if alias else ["cur_uv_out", "status_out"]) + (["iters"] if iters else [])
            _walk_entry(walk, E.klt_specs(k, n, run), inputs, lambda a: E.klt_call(F, D, walk.ctx, a, k, n, run),
                        ["ftk_klt_track_device"], written)
    inputs, _ = E.direct_case()
    written = [f"p{p}_{name}" for p in range(len(E.DIRECT_PROBLEMS)) for name in E.DIRECT_IN_OUT] + ["p0_iterations"]
    assert E.DIRECT_PROBLEMS == [(30, False, True), (31, True, False)] and "p0_status" not in inputs and "p1_status" in inputs
    _walk_entry(walk, E.direct_specs(), inputs, lambda a: E.direct_call(F, D, walk.ctx, a), ["ftk_direct_track_batch_device"], written)


def test_matcher_and_brief_specs_pass_the_entries_checks(walk):
    for n_ref, n_cur in E.MATCH_COUNTS:
        for nearby in (False, True):
            for n_bits in E.HAMMING_BITS:
                inputs, stale, _, thr = E.hamming_case(n_bits, n_ref, n_cur, nearby)
                for workspace in (True, False):
                    specs = E.hamming_specs(n_bits, n_ref, n_cur, nearby, workspace)
                    if workspace:
                        assert dict((s[0], s[2]) for s in specs)["workspace"] == (n_ref,)
                    written = ["index_pairs"] + (["workspace"] if workspace and n_ref > 1 else [])  # (two words are no fewer than the one needed)
                    _walk_entry(walk, specs, dict(inputs, index_pairs=stale), lambda a: E.hamming_call(D, walk.ctx, a, n_bits, thr, nearby, workspace),
                                ["ftk_hamming_match_device"], written)
            for dim in E.COSINE_DIMS:
                inputs, stale, _ = E.cosine_case(dim, n_ref, n_cur, nearby)
                _walk_entry(walk, E.cosine_specs(dim, n_ref, n_cur, nearby), dict(inputs, index_pairs=stale), lambda a: E.cosine_call(D, walk.ctx, a, nearby),
                            ["ftk_cosine_match_device"], ["index_pairs"])
    for n in E.BRIEF_COUNTS:
        for n_bits in E.BRIEF_BITS:
            for half in E.BRIEF_HALVES:
                _walk_entry(walk, E.brief_specs(n, n_bits), dict(image0=E.brief_image(), uv=E.brief_points(n)),
                            lambda a: E.brief_call(D, walk.ctx, a, n_bits, half), ["ftk_brief_compute_device"], ["words_out"])


def test_harris_and_table_specs_pass_the_entries_checks(walk, oracle):
    for size, distance, occupied in E.harris_runs():
        image, points, mask, survivors = E.harris_case(size, distance, occupied)
        inputs = dict(image0=image, **({} if points is None else dict(occupied=points)), **({} if mask is None else dict(occupied_mask=mask)))
        for max_count in E.harris_max_counts(len(survivors)):
            _walk_entry(walk, E.harris_specs(size, points, mask, max_count), inputs,
                        lambda a: E.harris_call(D, walk.ctx, a, distance, max_count, points is not None, mask is not None), ["ftk_harris_detect_device"],
                        ["uv_out", "count_out"])
    for n in E.TABLE_SIZES:
        for name, make, uv, status, back_uv, back_status, threshold in E.retire_cases(n):
            inputs = dict(E.table_state(make()), free_slots=np.full(n, E.FREE_STALE, np.int32), tracked_uv=uv, tracked_status=status)
            if back_uv is not None:
                inputs.update(back_uv=back_uv, back_status=back_status)
            _walk_entry(walk, E.table_specs(n, back_uv is not None), inputs, lambda a: E.retire_call(D, walk.ctx, a, threshold), ["ftk_track_table_retire_device"],
                        list(E.TABLE_STATE) + ["n_live", "free_slots", "n_free"])
        before, uv, status = E.TC.fill_state(n, (n + 1) // 2, 0)
        inputs = dict(E.table_state(before), free_slots=np.full(n, E.FREE_STALE, np.int32), tracked_uv=uv, tracked_status=status, next_id=before.next_id,
                      image0=E.TC.fill_image())
        _walk_entry(walk, E.table_specs(n, fill=True), inputs, lambda a: E.fill_call(D, walk.ctx, a), ["ftk_track_table_fill_device"],
                    list(E.TABLE_STATE) + ["n_live", "next_id", "free_slots", "n_free"])
    for case in range(len(E.MATCH_TABLE_CASES)):
        make, index, status, uv, desc, cur_count, q_count, max_lost, with_slot = E.match_table_case(case)
        inputs = dict(make().tensors(), match_index=index, match_status=status, cur_uv=uv, cur_desc=desc)
        if cur_count is not None:
            inputs["cur_count"] = np.array([cur_count], np.int32)
        specs = E.match_table_specs(case)
        _walk_entry(walk, specs, inputs, lambda a: E.match_query_call(D, walk.ctx, a), ["ftk_match_table_query_device"], ["q_uv", "q_desc", "q_slot", "q_count"])
        _walk_entry(walk, specs, inputs, lambda a: E.match_update_call(D, walk.ctx, a, max_lost, cur_count is not None, with_slot), ["ftk_match_table_update_device"],
                    list(E.TABLE_FIELDS) + ["workspace"] + (["cur_slot"] if with_slot else []))


def test_nn_and_dense_specs_pass_the_entries_checks(walk):
    for n_ref, n_cur in E.NN_SCORE_SHAPES:
        scores, _, _ = E.nn_scores_case(n_ref, n_cur)
        _walk_entry(walk, E.nn_scores_specs(n_ref, n_cur), dict(scores=scores), lambda a: E.nn_scores_call(D, walk.ctx, a), ["ftk_nn_match_scores_device"],
                    ["match_index", "status"], views=DeviceViews)
    for n_ref, n_cur in E.NN_LIST_SHAPES:
        matches, cur_uv, idx, _, _ = E.nn_list_case(n_ref, n_cur)
        specs = E.nn_list_specs(n_ref, n_cur)
        _walk_entry(walk, specs, dict(matches=matches, cur_uv=cur_uv), lambda a: E.nn_list_call(D, walk.ctx, a, n_ref, n_cur), ["ftk_nn_match_list_device"],
                    ["match_index", "status"], views=DeviceViews)
        _walk_entry(walk, specs, dict(matches=matches, cur_uv=cur_uv, match_index=idx), lambda a: E.nn_fill_call(D, walk.ctx, a), ["ftk_nn_fill_pixels_device"],
                    ["matched_uv"], views=DeviceViews)
    for w, h, levels in E.DENSE_CASES:
        inputs = E.dense_case(w, h, levels)[0]
        _walk_entry(walk, E.dense_specs(w, h, levels), inputs, lambda a: E.dense_call(F, D, walk.ctx, a, levels), ["ftk_dense_flow_device"], ["flow_r", "flow_c"])


def test_the_one_off_refusal_is_the_checks_own():
    """The walk's refusals come from the entries' checks, not from the stand-ins: an arena view is a plain dense tensor to ``_tensor_complaint``."""
    arena = _arena(E.hamming_specs(96, 65, 257, False, True), {})
    assert D._tensor_complaint("workspace", arena["workspace"], D._KEYS, (None,), 65) is None
    assert "too few" in D._tensor_complaint("workspace", arena["workspace"][:-1], D._KEYS, (None,), 65)
    assert TR.survivor_bound(23, 23, 1) > 0
