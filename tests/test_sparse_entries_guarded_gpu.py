"""The torch-facing device entries of the sparse tracker, held to their tensors on guarded memory (tests/guarded.py): ``DeviceKlt.track`` /
``.bind``, ``DeviceDirectBatch.track``, ``hamming_match_device``, ``cosine_match_device``, ``brief_compute_device``, ``harris_detect_device``,
``track_table_retire_device`` / ``track_table_fill_device``, ``match_table_query_device`` / ``match_table_update_device``,
``nn_match_scores_device`` / ``nn_match_list_device`` / ``nn_fill_pixels_device`` and ``dense_flow_device``, called directly, not through
the classes that own staging blocks and workspaces with room to spare:

 (a) every tensor a call may write is a guarded payload of exactly its documented shape or element count; a workspace is exactly
     ``ceil(*_workspace_bytes / 8)`` int64 words, ``hamming_match_device``'s exactly ``n_ref`` words;
 (b) every tensor a call only reads (the pyramid levels included: the pyramids are ``pyramid_from_tensors`` over payloads) is a payload too,
     and holds its bytes after the call;
 (c) every call is made on two fresh arenas, all payloads 0x00 and all payloads 0xFF, and both results equal the oracle or the restatement
     bit for bit;
 (d) no guard band is written;
 (e) every payload starts 256-byte aligned, as a block of torch's allocator does (misaligned views: part B of tests/test_device_args_gpu.py).

(c) with the two kinds of tensor this family has.  A PURE OUTPUT keeps the arena's fill before the call and is equal after both.  An
IN/OUT tensor gets its input ``put`` after the fill, so both runs start from the same content and must end equal to the restatement applied
to it.  Per entry (the contract: INTEGRATION.md, DESIGN.md 5.1, 5.3, 5.11, 5.19, 5.28, the entries' docstrings):

 KLT            pure: ``cur_uv_out``, ``status_out``, ``iters`` (a passed-through or capped feature gets its incoming position and status
                and 0 iterations written, DeviceKlt.track's docstring).  in/out: ``cur_uv_in`` / ``status_in`` when the out tensors alias them.
 direct batch   in/out: ``cur_uv``, ``pose``, and ``status`` of a problem with ``status_valid``.  pure: ``status`` without it, ``iterations``.
 matchers       in/out: ``index_pairs`` (an entry without a match keeps what it held).  pure: the Hamming ``workspace``.
 BRIEF          pure: ``words_out``, the all-zero rows of features at the border and the unused bits of a partial last word included
                (include/ftk.h: such features GET all-zero words).
 masked Harris  pure: ``uv_out`` (zeros behind the count) and ``count_out``.
 track table    retire: in/out ``ids``, ``points``, ``prev_points``, ``status``, ``age`` (an empty slot is not touched) and ``free_slots``
                (nothing behind ``n_free`` is written); pure ``n_live`` and ``n_free``.  fill: in/out the five, ``n_live`` and ``next_id``;
                ``free_slots`` and ``n_free`` are only read.
 match table    query: pure ``q_uv``, ``q_desc``, ``q_slot``, ``q_count`` (+0 and -1 behind the count).  update: in/out the nine table
                tensors; pure ``workspace`` and ``cur_slot``.
 NN             pure: ``match_index``, ``status``, ``matched_uv``.
 dense flow     pure: ``flow_r``, ``flow_c``.

The KLT option sets name the launch form ``klt_plan`` must choose for them; tests/test_sparse_entries_guarded_cpu.py walks the plan, holds
every set to its form, derives the feature counts 1, g, g + 1 and an odd count of a few workgroups from the plan's features per workgroup g
(``klt_counts``: no count is written down here), holds the other shape lists to the tails they claim, and runs every spec list below
through the entries' argument checks on CPU tensors.  The tail class is pinned per set (FTK_KLT_TAIL_CLASS), because the plan follows it
and the library would otherwise take it from the timing of earlier calls.  No kernel is run out of bounds here.

Not covered: the sharded entries (``track_sharded``, ``bind_sharded``, ``track_shard``, ``unpack_shards``, ``hamming_match_sharded_device``).

The case lists, spec lists and calls below take the package, the device module and the device as arguments: the CPU file builds the same
arenas on CPU tensors."""
import functools

import numpy as np
import pytest

from feature_tracker_amd import synth
from tests import dense_flow_ref as DR
from tests import guarded as G
from tests import match_table_cases as MC
from tests import nn_match_ref as NR
from tests import scenes
from tests import track_table_cases as TC
from tests import track_table_ref as TR
from tests.test_device_args_gpu import _positions, dev_ctx  # noqa: F401  (the fixture: a context on a torch stream, that stream current)
from tests.test_direct_method_gpu import CX, CY, FX, FY
from tests.test_direct_method_gpu import scene as direct_scene
from tests.test_harris_device_gpu import MIN_RESPONSE as HARRIS_MIN_RESPONSE
from tests.test_harris_device_gpu import _scene as harris_scene
from tests.test_harris_device_gpu import occupied_sets

pytestmark = pytest.mark.gpu

FILLS = (G.ZEROS, G.ONES)
_TORCH_NAME = {np.dtype(np.float32): "float32", np.dtype(np.uint8): "uint8", np.dtype(np.int32): "int32", np.dtype(np.uint32): "int32",
               np.dtype(np.int64): "int64"}


def _readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _spec(name, shape, dtype="float32"):
    return (name, dtype, tuple(int(e) for e in shape), 0)


def _like(name, array):
    return _spec(name, array.shape, _TORCH_NAME[array.dtype])


def make_arena(specs, inputs, fill, device="cuda"):
    arena = G.Arena(specs, device, fill=fill)
    for name, array in inputs.items():
        arena.put(name, array)
    return arena


def _finish(arena, readonly):
    """(d) and (b) after the call: one synchronisation, one copy of the arena, every guard intact, every input as it was."""
    import torch
    torch.cuda.synchronize()
    host = arena.check()
    for name, array in readonly.items():
        assert arena.payload_bytes(name, host).tobytes() == np.ascontiguousarray(array).tobytes(), f"the call changed its input {name}"
    return host


def _np(arena, name):
    return arena[name].cpu().numpy()


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize and got.tobytes() == want.tobytes()


def level_specs(prefix, levels):
    return [_spec(f"{prefix}{i}", l.shape, "uint8") for i, l in enumerate(levels)]


def level_inputs(prefix, levels):
    return {f"{prefix}{i}": np.ascontiguousarray(l) for i, l in enumerate(levels)}


def pyramid(D, ctx, arena, prefix, count):
    """The pyramid whose levels are the payloads ``prefix0 .. prefix{count - 1}``: borrowed, not copied."""
    return D.pyramid_from_tensors([arena[f"{prefix}{i}"] for i in range(count)], ctx)


# ---- DeviceKlt.track and .bind ------------------------------------------------------------------------------------------------------------
# (name, model, method, consider_luminance, half patch, FTK_KLT_TAIL_CLASS, (width, height, levels), the form klt_plan must choose).  The
# large patch is tests/test_klt_gpu.py's: half 30 of the affine inverse tracker on the 640 x 480 scene of two levels.
KLT_SETS = [
    ("basic/inverse", "basic", "inverse", False, 5, 0, (160, 120, 3), "pipelined"),            # a feature on several waves, one per workgroup
    ("basic/inverse, one wave", "basic", "inverse", False, 5, 1, (160, 120, 3), "pipelined"),  # the solo form: several features per workgroup
    ("basic/fast", "basic", "fast", False, 5, 0, (160, 120, 3), "one_wave_fast"),
    ("affine/fast", "affine", "fast", False, 5, 0, (160, 120, 3), "one_wave_fast"),
    ("basic/direct", "basic", "direct", False, 5, 0, (160, 120, 3), "generic"),
    ("affine/inverse", "affine", "inverse", False, 5, 0, (160, 120, 3), "generic"),
    ("affine/direct", "affine", "direct", False, 5, 0, (160, 120, 3), "generic"),
    ("lssd/inverse", "lssd", "inverse", False, 5, 0, (160, 120, 3), "generic"),
    ("lssd/inverse, luminance", "lssd", "inverse", True, 5, 0, (160, 120, 3), "generic"),
    ("lssd/direct", "lssd", "direct", False, 5, 0, (160, 120, 3), "generic"),
    ("lssd/fast", "lssd", "fast", False, 5, 0, (160, 120, 3), "generic"),                       # the chunked level form
    ("lssd/fast, luminance", "lssd", "fast", True, 5, 0, (160, 120, 3), "generic"),
    ("affine/inverse, large patch", "affine", "inverse", False, 30, 0, (640, 480, 2), "generic_spill"),
]
KLT_OPTION_CAP = 100  # kMaxTrackPointsNumber of the options: above every count here
# name -> (iters given, max_track_points below n, the out tensors alias the in tensors, through bind)
KLT_RUNS = {"track": (True, False, False, False), "capped, no iters": (False, True, False, False), "aliased": (True, True, True, False),
            "bind": (True, False, False, True)}
KLT_RUNS_AT_EVERY_COUNT = ("track", "capped, no iters")  # the other two once per set, at its largest count


def klt_counts(k):
    """(g, (1, g, g + 1, an odd count of a few workgroups)) of KLT_SETS[k]: g is the plan's features per workgroup, asked of the host plan
    program by the CPU file, which also holds the counts to these properties."""
    from tests import test_sparse_entries_guarded_cpu as P
    return P.klt_counts(k)


def klt_cap(n):
    """The cap of a capped run: the last feature is beyond it (no cap is below one feature)."""
    return n - 1 if n > 1 else 1


def klt_features(k):
    _, _, _, _, half, _, (w, h, _), _ = KLT_SETS[k]
    if half > 6:
        return scenes.features(24, w, h, half=half, border_fraction=0.1)
    return scenes.features(16, w, h, half=half)


@functools.lru_cache(maxsize=None)
def klt_case(k, n, capped):
    """(inputs by payload name, the oracle's (cur_uv, status, iters)): some features arrive with a status above tracked, the start
    positions differ from the reference positions, so that a passed-through slot shows where its output came from."""
    from tests import oracle_lib
    _, model, method, lum, half, _, (w, h, levels), _ = KLT_SETS[k]
    ref_levels, cur_levels = scenes.scene(w, h, levels)
    uv = np.ascontiguousarray(klt_features(k)[:n])
    assert len(uv) == n
    start = (uv + np.float32([0.5, -0.25])).astype(np.float32)
    status = ((np.arange(n) % 5 == 3) * 3).astype(np.uint8)
    ok, c, s, it = oracle_lib.klt_track_pyramid(model, ref_levels, cur_levels, uv, start.copy(), status.copy(), consider_luminance=lum, method=method,
                                               half=half, max_points=klt_cap(n) if capped else KLT_OPTION_CAP)
    assert ok
    inputs = dict(level_inputs("ref", ref_levels), **level_inputs("cur", cur_levels), ref_uv=uv, cur_uv_in=start, status_in=status)
    want = (np.ascontiguousarray(c, np.float32), np.ascontiguousarray(s, np.uint8), np.asarray(it, np.uint32))
    _readonly(*want, *inputs.values())
    return inputs, want


def klt_specs(k, n, run):
    iters, _, alias, _ = KLT_RUNS[run]
    _, _, _, _, _, _, (w, h, levels), _ = KLT_SETS[k]
    ref_levels, cur_levels = scenes.scene(w, h, levels)
    specs = level_specs("ref", ref_levels) + level_specs("cur", cur_levels)
    specs += [_spec("ref_uv", (n, 2)), _spec("cur_uv_in", (n, 2)), _spec("status_in", (n,), "uint8")]
    if not alias:
        specs += [_spec("cur_uv_out", (n, 2)), _spec("status_out", (n,), "uint8")]
    if iters:
        specs.append(_spec("iters", (n,), "int32"))
    return specs


def klt_call(F, D, ctx, arena, k, n, run):
    iters, capped, alias, bind = KLT_RUNS[run]
    _, model, method, lum, half, _, (_, _, levels), _ = KLT_SETS[k]
    opt = F.OpticalFlowOptions()
    opt.kMethod, opt.kPatchRowHalfSize, opt.kPatchColHalfSize, opt.kMaxTrackPointsNumber = method, half, half, KLT_OPTION_CAP
    klt = D.DeviceKlt(model, opt, pyramid(D, ctx, arena, "ref", levels), pyramid(D, ctx, arena, "cur", levels), ctx, consider_luminance=lum)
    out, status_out = (arena["cur_uv_in"], arena["status_in"]) if alias else (arena["cur_uv_out"], arena["status_out"])
    args = (arena["ref_uv"], arena["cur_uv_in"], arena["status_in"], out, status_out, arena["iters"] if iters else None)
    if bind:
        assert not capped
        klt.bind(*args)()
    else:
        klt.track(*args, max_track_points=klt_cap(n) if capped else None)


def klt_runs(k):
    """Every (n, run) of a set."""
    _, counts = klt_counts(k)
    return [(n, run) for n in counts for run in KLT_RUNS_AT_EVERY_COUNT] + [(max(counts), run) for run in KLT_RUNS if run not in KLT_RUNS_AT_EVERY_COUNT]


@pytest.mark.parametrize("k", range(len(KLT_SETS)), ids=[s[0] for s in KLT_SETS])
def test_klt_on_guarded_memory(ftk, oracle, dev_ctx, switch, k):  # noqa: F811
    g = dev_ctx
    switch("FTK_KLT_TAIL_CLASS", str(KLT_SETS[k][5]))
    for n, run in klt_runs(k):
        iters, capped, alias, _ = KLT_RUNS[run]
        inputs, (want_uv, want_status, want_iters) = klt_case(k, n, capped)
        readonly = {name: a for name, a in inputs.items() if not (alias and name in ("cur_uv_in", "status_in"))}
        for fill in FILLS:
            arena = make_arena(klt_specs(k, n, run), inputs, fill)
            klt_call(ftk, g.D, g.ctx, arena, k, n, run)
            _finish(arena, readonly)
            what = (KLT_SETS[k][0], n, run, hex(fill))
            got_uv, got_status = (_np(arena, "cur_uv_in"), _np(arena, "status_in")) if alias else (_np(arena, "cur_uv_out"), _np(arena, "status_out"))
            assert np.array_equal(got_status, want_status), (what, got_status, want_status)
            assert _same(got_uv, want_uv), (what, got_uv, want_uv)
            if iters:
                assert np.array_equal(_np(arena, "iters").view(np.uint32), want_iters), (what, _np(arena, "iters"), want_iters)
        if capped and n > 1:  # the capped slot exists, and a passed-through one from three features on: their outputs are their inputs
            assert _same(want_uv[-1], inputs["cur_uv_in"][-1]) and want_status[-1] == inputs["status_in"][-1] and want_iters[-1] == 0


# ---- DeviceDirectBatch.track ----------------------------------------------------------------------------------------------------------------
# two problems of 30 and 31 points on one pair of pyramids (320 x 240, three levels): (points, status_valid, iterations given)
DIRECT_PROBLEMS = [(30, False, True), (31, True, False)]
DIRECT_LEVELS = 3


@functools.lru_cache(maxsize=None)
def direct_case():
    """(inputs by payload name, per problem the oracle's (cur_uv, pose, status, iterations))."""
    from tests import oracle_lib
    rl, cl, uv_all, pts_all = direct_scene(w=320, h=240, levels=DIRECT_LEVELS, n=31)
    inputs, want = dict(level_inputs("ref", rl), **level_inputs("cur", cl)), []
    for p, (n, status_valid, _) in enumerate(DIRECT_PROBLEMS):
        uv, pts = np.ascontiguousarray(uv_all[31 - n:]), np.ascontiguousarray(pts_all[31 - n:])
        status = ((np.arange(n) % 7 == 2) * 3).astype(np.uint8) if status_valid else None
        ok, c, q, t, st, it = oracle_lib.direct_track(rl, cl, [FX, FY, CX, CY], pts, uv, status=None if status is None else status.copy())
        assert ok and it > 0
        inputs.update({f"p{p}_p_c_in_ref": pts, f"p{p}_ref_uv": uv, f"p{p}_cur_uv": uv.copy(), f"p{p}_pose": np.float32([1, 0, 0, 0, 0, 0, 0])})
        if status_valid:
            inputs[f"p{p}_status"] = status
        want.append((np.ascontiguousarray(c, np.float32), np.concatenate([np.float32(q), np.float32(t)]), np.ascontiguousarray(st, np.uint8), int(it)))
    _readonly(*inputs.values())
    return inputs, want


DIRECT_IN_OUT = ("cur_uv", "pose", "status")


def direct_specs():
    rl, cl, _, _ = direct_scene(w=320, h=240, levels=DIRECT_LEVELS, n=31)
    specs = level_specs("ref", rl) + level_specs("cur", cl)
    for p, (n, _, iterations) in enumerate(DIRECT_PROBLEMS):
        specs += [_spec(f"p{p}_p_c_in_ref", (n, 3)), _spec(f"p{p}_ref_uv", (n, 2)), _spec(f"p{p}_cur_uv", (n, 2)), _spec(f"p{p}_pose", (7,)),
                  _spec(f"p{p}_status", (n,), "uint8")]
        if iterations:
            specs.append(_spec(f"p{p}_iterations", (1,), "int32"))
    return specs


def direct_call(F, D, ctx, arena):
    rp, cp = pyramid(D, ctx, arena, "ref", DIRECT_LEVELS), pyramid(D, ctx, arena, "cur", DIRECT_LEVELS)
    problems = []
    for p, (n, status_valid, iterations) in enumerate(DIRECT_PROBLEMS):
        problems.append(dict(ref=rp, cur=cp, K=[FX, FY, CX, CY], p_c_in_ref=arena[f"p{p}_p_c_in_ref"], ref_uv=arena[f"p{p}_ref_uv"], cur_uv=arena[f"p{p}_cur_uv"],
                             pose=arena[f"p{p}_pose"], status=arena[f"p{p}_status"], status_valid=status_valid,
                             iterations=arena[f"p{p}_iterations"] if iterations else None))
    D.DeviceDirectBatch(F.DirectMethodOptions(), problems, ctx).track()


def test_direct_batch_on_guarded_memory(ftk, oracle, dev_ctx):  # noqa: F811
    g = dev_ctx
    inputs, want = direct_case()
    readonly = {name: a for name, a in inputs.items() if name.split("_", 1)[-1] not in DIRECT_IN_OUT}
    for fill in FILLS:
        arena = make_arena(direct_specs(), inputs, fill)
        direct_call(ftk, g.D, g.ctx, arena)
        _finish(arena, readonly)
        for p, (uv, pose, status, it) in enumerate(want):
            what = (p, hex(fill))
            assert _same(_np(arena, f"p{p}_pose"), pose), (what, _np(arena, f"p{p}_pose"), pose)
            assert _same(_np(arena, f"p{p}_cur_uv"), uv), what
            assert np.array_equal(_np(arena, f"p{p}_status"), status), what
            if DIRECT_PROBLEMS[p][2]:
                assert int(_np(arena, f"p{p}_iterations")[0]) == it, what


# ---- hamming_match_device and cosine_match_device ----------------------------------------------------------------------------------------------
MATCH_COUNTS = [(65, 257), (1, 1)]   # (n_ref, n_cur): a tail on both axes of every form's tiles; one row against one row
HAMMING_BITS = {256: (20, 60.0), 96: (7, 25.0), 32: (2, 8.0)}  # n_bits -> (flipped bits of a true pair, max_distance): 8 words (MFMA), 3, 1
COSINE_DIMS = (256, 100)
STALE = 5000


def _unmatched(n_ref):
    """The reference rows that are spoiled, so that they find no match and ``index_pairs`` must keep what it held there."""
    return np.arange(n_ref) % 8 == 5


@functools.lru_cache(maxsize=None)
def hamming_case(n_bits, n_ref, n_cur, nearby):
    from feature_tracker_amd import pack_brief
    from tests import oracle_lib
    flips, thr = HAMMING_BITS[n_bits]
    ref, cur, perm = synth.make_descriptors(n_ref, n_cur, n_bits=n_bits, flips=flips)
    ref[_unmatched(n_ref)] ^= 1  # every bit: n_bits - flips from its pair
    pred_uv, cur_uv = _positions(n_ref, n_cur, perm)
    stale = np.arange(n_ref, dtype=np.int32) + STALE
    if nearby:
        ok, want = oracle_lib.nearby_match(ref, cur, pred_uv, cur_uv, thr, 40, 40, stale.copy())
    else:
        ok, want = oracle_lib.force_match(ref, cur, thr, stale.copy())
    assert ok
    inputs = dict(ref_words=pack_brief(ref), cur_words=pack_brief(cur))
    if nearby:
        inputs.update(pred_uv=pred_uv, cur_uv=cur_uv)
    want = np.ascontiguousarray(want, np.int32)
    _readonly(want, stale, *inputs.values())
    return inputs, stale, want, thr


def hamming_specs(n_bits, n_ref, n_cur, nearby, workspace):
    words = (n_bits + 31) // 32
    specs = [_spec("ref_words", (n_ref, words), "int32"), _spec("cur_words", (n_cur, words), "int32"), _spec("index_pairs", (n_ref,), "int32")]
    if nearby:
        specs += [_spec("pred_uv", (n_ref, 2)), _spec("cur_uv", (n_cur, 2))]
    if workspace:
        specs.append(_spec("workspace", (n_ref,), "int64"))  # exactly n_ref words
    return specs


def hamming_call(D, ctx, arena, n_bits, thr, nearby, workspace):
    kw = dict(pred_uv=arena["pred_uv"], cur_uv=arena["cur_uv"]) if nearby else {}
    D.hamming_match_device(ctx, arena["ref_words"], arena["cur_words"], n_bits, thr, arena["index_pairs"], workspace=arena["workspace"] if workspace else None, **kw)


@pytest.mark.parametrize("nearby", [False, True], ids=["force", "nearby"])
@pytest.mark.parametrize("n_bits", sorted(HAMMING_BITS, reverse=True))
def test_hamming_on_guarded_memory(ftk, oracle, dev_ctx, n_bits, nearby):  # noqa: F811
    g = dev_ctx
    for n_ref, n_cur in MATCH_COUNTS:
        inputs, stale, want, thr = hamming_case(n_bits, n_ref, n_cur, nearby)
        for workspace in (True, False):
            for fill in FILLS:
                arena = make_arena(hamming_specs(n_bits, n_ref, n_cur, nearby, workspace), dict(inputs, index_pairs=stale), fill)
                hamming_call(g.D, g.ctx, arena, n_bits, thr, nearby, workspace)
                _finish(arena, inputs)
                got = _np(arena, "index_pairs")
                assert np.array_equal(got, want), ((n_ref, n_cur), workspace, hex(fill), np.flatnonzero(got != want)[:5])


@functools.lru_cache(maxsize=None)
def cosine_case(dim, n_ref, n_cur, nearby):
    from tests import oracle_lib
    ref, cur, perm = synth.make_float_descriptors(n_ref, n_cur, dim=dim)
    ref[_unmatched(n_ref)] *= np.float32(-1.0)  # cosine distance 2 - d from its pair
    pred_uv, cur_uv = _positions(n_ref, n_cur, perm)
    stale = np.arange(n_ref, dtype=np.int32) + STALE
    ok, want = oracle_lib.match_float(ref, cur, 0.3, pred_uv if nearby else None, cur_uv if nearby else None, 40, 40, stale.copy())
    assert ok
    inputs = dict(ref_desc=ref, cur_desc=cur)
    if nearby:
        inputs.update(pred_uv=pred_uv, cur_uv=cur_uv)
    want = np.ascontiguousarray(want, np.int32)
    _readonly(want, stale, *inputs.values())
    return inputs, stale, want


def cosine_specs(dim, n_ref, n_cur, nearby):
    specs = [_spec("ref_desc", (n_ref, dim)), _spec("cur_desc", (n_cur, dim)), _spec("index_pairs", (n_ref,), "int32")]
    return specs + ([_spec("pred_uv", (n_ref, 2)), _spec("cur_uv", (n_cur, 2))] if nearby else [])


def cosine_call(D, ctx, arena, nearby):
    kw = dict(pred_uv=arena["pred_uv"], cur_uv=arena["cur_uv"]) if nearby else {}
    D.cosine_match_device(ctx, arena["ref_desc"], arena["cur_desc"], 0.3, arena["index_pairs"], **kw)


@pytest.mark.parametrize("small", [None, "0"], ids=["default", "launches"])
@pytest.mark.parametrize("dim", COSINE_DIMS)
def test_cosine_on_guarded_memory(ftk, oracle, dev_ctx, switch, dim, small):  # noqa: F811
    g = dev_ctx
    if small is not None:
        switch("FTK_COSINE_SMALL", small)
    for n_ref, n_cur in MATCH_COUNTS:
        for nearby in (False, True):
            inputs, stale, want = cosine_case(dim, n_ref, n_cur, nearby)
            for fill in FILLS:
                arena = make_arena(cosine_specs(dim, n_ref, n_cur, nearby), dict(inputs, index_pairs=stale), fill)
                cosine_call(g.D, g.ctx, arena, nearby)
                _finish(arena, inputs)
                got = _np(arena, "index_pairs")
                assert np.array_equal(got, want), ((n_ref, n_cur), nearby, hex(fill), np.flatnonzero(got != want)[:5])


# ---- brief_compute_device ------------------------------------------------------------------------------------------------------------------
BRIEF_BITS = (256, 100, 32)   # 8 words; 4 words of which the last holds 4 bits; 1 word
BRIEF_COUNTS = (1, 65)
BRIEF_HALVES = (8, 63)        # the usual patch and the largest the entry takes
BRIEF_IMAGE = (320, 240)


@functools.lru_cache(maxsize=None)
def brief_image():
    return _readonly(np.ascontiguousarray(synth.make_image_pair(*BRIEF_IMAGE)[0]))[0]


@functools.lru_cache(maxsize=None)
def brief_points(n):
    """Points 70 pixels and more inside the image (a descriptor at both half patches); of 65, four at or beyond the border (all-zero rows)."""
    w, h = BRIEF_IMAGE
    rs = np.random.RandomState(n)
    uv = np.stack([rs.uniform(70, w - 71, n), rs.uniform(70, h - 71, n)], axis=1).astype(np.float32)
    if n > 10:
        uv[3], uv[10], uv[-1], uv[-2] = (2.0, 5.0), (100.0, h - 1.5), (w - 1.0, 120.0), (-4.0, 300.0)
    return _readonly(uv)[0]


@functools.lru_cache(maxsize=None)
def brief_want(n, n_bits, half):
    from feature_tracker_amd import pack_brief
    from tests import oracle_lib
    ok, bits = oracle_lib.brief_compute(brief_image(), brief_points(n), n_bits, half)
    assert ok
    return _readonly(pack_brief(bits))[0]


def brief_specs(n, n_bits):
    return [_like("image0", brief_image()), _spec("uv", (n, 2)), _spec("words_out", (n, (n_bits + 31) // 32), "int32")]


def brief_call(D, ctx, arena, n_bits, half):
    D.brief_compute_device(ctx, pyramid(D, ctx, arena, "image", 1), arena["uv"], n_bits, half, arena["words_out"])


@pytest.mark.parametrize("half", BRIEF_HALVES)
@pytest.mark.parametrize("n_bits", BRIEF_BITS)
def test_brief_on_guarded_memory(ftk, oracle, dev_ctx, n_bits, half):  # noqa: F811
    g = dev_ctx
    for n in BRIEF_COUNTS:
        inputs = dict(image0=brief_image(), uv=brief_points(n))
        want = brief_want(n, n_bits, half)
        for fill in FILLS:
            arena = make_arena(brief_specs(n, n_bits), inputs, fill)
            brief_call(g.D, g.ctx, arena, n_bits, half)
            _finish(arena, inputs)
            got = _np(arena, "words_out").view(np.uint32)
            assert np.array_equal(got, want), (n, hex(fill), np.argwhere(got != want)[:5].tolist())


# ---- harris_detect_device ------------------------------------------------------------------------------------------------------------------
HARRIS_CASES = [((23, 23), 1), ((64, 48), 2), ((333, 251), 2)]  # ((width, height), min_distance); 23 x 23 has one valid centre
HARRIS_OCCUPIED = ("none", "dense_random", "on_the_strongest")     # no points; 200 points under a mask; the strongest corner blocked (no mask)


@functools.lru_cache(maxsize=None)
def harris_case(size, distance, occupied):
    """(image, points or None, mask or None, every survivor strongest first)."""
    image = harris_scene(*size)
    points, mask = occupied_sets(image, distance).get(occupied, (None, None))
    survivors = TR.masked_survivors(image, distance, HARRIS_MIN_RESPONSE, points, mask)
    return _readonly(image)[0], points, mask, survivors


def harris_max_counts(S):
    return sorted({c for c in (S - 1, S, S + 3) if c >= 1})


def harris_runs():
    runs = []
    for size, distance in HARRIS_CASES:
        for occupied in HARRIS_OCCUPIED:
            if occupied == "none" or occupied in occupied_sets(harris_scene(*size), distance):
                runs.append((size, distance, occupied))
    return runs


def harris_specs(size, occupied_points, mask, max_count):
    specs = [_spec("image0", (size[1], size[0]), "uint8")]
    if occupied_points is not None:
        specs.append(_spec("occupied", occupied_points.shape))
    if mask is not None:
        specs.append(_spec("occupied_mask", mask.shape, "uint8"))
    return specs + [_spec("uv_out", (max_count, 2)), _spec("count_out", (1,), "int32")]


def harris_call(D, ctx, arena, distance, max_count, with_points, with_mask):
    D.harris_detect_device(ctx, pyramid(D, ctx, arena, "image", 1), max_count, distance, HARRIS_MIN_RESPONSE, arena["uv_out"], arena["count_out"],
                           arena["occupied"] if with_points else None, arena["occupied_mask"] if with_mask else None)


@pytest.mark.parametrize("size,distance", HARRIS_CASES, ids=str)
def test_masked_harris_on_guarded_memory(ftk, oracle, dev_ctx, size, distance):  # noqa: F811
    g = dev_ctx
    for _, _, occupied in [r for r in harris_runs() if r[0] == size]:
        image, points, mask, survivors = harris_case(size, distance, occupied)
        inputs = dict(image0=image)
        if points is not None:
            inputs["occupied"] = points
        if mask is not None:
            inputs["occupied_mask"] = mask
        for max_count in harris_max_counts(len(survivors)):
            want_uv, want_count = TR.detect(image, max_count, distance, HARRIS_MIN_RESPONSE, points, mask)
            for fill in FILLS:
                arena = make_arena(harris_specs(size, points, mask, max_count), inputs, fill)
                harris_call(g.D, g.ctx, arena, distance, max_count, points is not None, mask is not None)
                _finish(arena, inputs)
                what = (occupied, max_count, len(survivors), hex(fill))
                assert int(_np(arena, "count_out")[0]) == want_count, (what, _np(arena, "count_out"))
                assert _same(_np(arena, "uv_out"), want_uv), what  # the zeros behind the count too: from the 0xFF fill they were written


# ---- track_table_retire_device and track_table_fill_device ----------------------------------------------------------------------------------------
TABLE_SIZES = (1, 255, 256, 257, 1025)
TABLE_PATTERNS = ("random", "every_status", "all_empty", "all_dead")
TABLE_STATE = ("ids", "points", "prev_points", "status", "age")
TABLE_DTYPES = {"ids": "int64", "points": "float32", "prev_points": "float32", "status": "uint8", "age": "int32", "n_live": "int32", "next_id": "int64"}
FREE_STALE = 0x7C7C7C7C  # what free_slots holds before retire: nothing behind n_free may change


def table_specs(n, forward_backward=False, fill=False):
    specs = [_spec(name, (n, 2) if "points" in name else (n,), TABLE_DTYPES[name]) for name in TABLE_STATE]
    specs += [_spec("n_live", (1,), "int32"), _spec("tracked_uv", (n, 2)), _spec("tracked_status", (n,), "uint8")]
    if forward_backward:
        specs += [_spec("back_uv", (n, 2)), _spec("back_status", (n,), "uint8")]
    specs += [_spec("free_slots", (n,), "int32"), _spec("n_free", (1,), "int32")]
    if fill:
        specs += [_spec("next_id", (1,), "int64")] + level_specs("image", [TC.fill_image()])
    return specs


def table_state(table):
    return {name: getattr(table, name).copy() for name in TABLE_STATE}


def retire_call(D, ctx, arena, forward_backward=None):
    a = arena
    D.track_table_retire_device(ctx, a["ids"], a["points"], a["prev_points"], a["status"], a["age"], a["n_live"], a["tracked_uv"], a["tracked_status"],
                                a["free_slots"], a["n_free"], a["back_uv"] if forward_backward is not None else None,
                                a["back_status"] if forward_backward is not None else None, 0.0 if forward_backward is None else forward_backward)


def fill_call(D, ctx, arena):
    a = arena
    D.track_table_fill_device(ctx, pyramid(D, ctx, arena, "image", 1), TC.FILL_MIN_DISTANCE, TC.FILL_MIN_RESPONSE, a["ids"], a["points"], a["prev_points"],
                              a["status"], a["age"], a["n_live"], a["next_id"], a["free_slots"], a["n_free"])


def retire_cases(n):
    """(name, a function that makes the table before the call, tracked_uv, tracked_status, back_uv, back_status, threshold)."""
    cases = []
    for k, pattern in enumerate(TABLE_PATTERNS):
        make = functools.partial(TC.state, n, k, TC.held_mode(pattern))
        cases.append((pattern, make, TC.tracked_points(n, k), TC.outcome(make(), pattern, k), None, None, None))
    make = functools.partial(TC.fb_state, n, 0)
    tracked_status, back_uv, back_status, _ = TC.forward_backward(make(), 0)
    cases.append(("forward-backward", make, TC.tracked_points(n, 0), tracked_status, back_uv, back_status, 1.0))
    return cases


def _table_equal(arena, table, what):
    for name in TABLE_STATE:
        assert _same(_np(arena, name), getattr(table, name)), (what, name)
    assert int(_np(arena, "n_live")[0]) == int(table.n_live[0]), (what, "n_live")


def _free_list_equal(arena, free, n, what):
    assert int(_np(arena, "n_free")[0]) == len(free), (what, _np(arena, "n_free"), len(free))
    want = np.full(n, FREE_STALE, np.int32)
    want[:len(free)] = free
    assert np.array_equal(_np(arena, "free_slots"), want), (what, "free_slots")


@pytest.mark.parametrize("n", TABLE_SIZES)
def test_track_table_retire_on_guarded_memory(ftk, oracle, dev_ctx, n):  # noqa: F811
    g = dev_ctx
    for name, make, tracked_uv, tracked_status, back_uv, back_status, threshold in retire_cases(n):
        before = make()
        readonly = dict(tracked_uv=tracked_uv, tracked_status=tracked_status)
        if back_uv is not None:
            readonly.update(back_uv=back_uv, back_status=back_status)
        after = make()
        free = after.retire(tracked_uv, tracked_status, back_uv, back_status, threshold)
        for fill in FILLS:
            arena = make_arena(table_specs(n, back_uv is not None), dict(table_state(before), free_slots=np.full(n, FREE_STALE, np.int32), **readonly), fill)
            retire_call(g.D, g.ctx, arena, threshold)
            _finish(arena, readonly)
            what = (name, hex(fill))
            _table_equal(arena, after, what)
            _free_list_equal(arena, free, n, what)


@pytest.mark.parametrize("n", TABLE_SIZES)
def test_track_table_retire_then_fill_on_guarded_memory(ftk, oracle, dev_ctx, n):  # noqa: F811
    """Half of the slots end empty; fill puts the masked survivors of the fill image into them and leaves the free list as it read it."""
    g = dev_ctx
    n_free = (n + 1) // 2
    before, tracked_uv, tracked_status = TC.fill_state(n, n_free, 0)
    after, _, _ = TC.fill_state(n, n_free, 0)
    free = list(after.retire(tracked_uv, tracked_status))
    assert len(free) == n_free
    retired = {name: getattr(after, name).copy() for name in TABLE_STATE + ("n_live",)}
    filled = after.detect_and_fill(TC.fill_image(), TC.FILL_MIN_DISTANCE, TC.FILL_MIN_RESPONSE)
    assert 1 <= filled <= n_free
    readonly = dict(tracked_uv=tracked_uv, tracked_status=tracked_status, image0=TC.fill_image())
    for fill in FILLS:
        arena = make_arena(table_specs(n, fill=True), dict(table_state(before), free_slots=np.full(n, FREE_STALE, np.int32), next_id=before.next_id, **readonly), fill)
        retire_call(g.D, g.ctx, arena)
        host = _finish(arena, dict(readonly, next_id=before.next_id))
        for name in TABLE_STATE + ("n_live",):
            assert _same(_np(arena, name), retired[name]), (hex(fill), "retire", name)
        _free_list_equal(arena, free, n, (hex(fill), "retire"))
        listed = {name: arena.payload_bytes(name, host).copy() for name in ("free_slots", "n_free")}
        fill_call(g.D, g.ctx, arena)
        _finish(arena, dict(readonly, **listed))  # fill reads the free list and writes none of it
        _table_equal(arena, after, (hex(fill), "fill"))
        assert int(_np(arena, "next_id")[0]) == int(after.next_id[0]) == int(before.next_id[0]) + filled, hex(fill)


# ---- match_table_query_device and match_table_update_device -----------------------------------------------------------------------------------------
# the smallest cases with a tail on the slot axis and on the current-row axis: a hand-written scenario of 5 slots against 3 rows (one
# partial group of the four flags a thread scans, one partial workgroup of the four-row movers), and a random frame of 65 slots against
# 67 rows (one wave and one slot, one wave and three rows), with and without cur_count and cur_slot
MATCH_TABLE_CASES = [("two rows name one j", None, None), ("random", True, False), ("random", False, True)]
MATCH_TABLE_RANDOM = (65, 67, 4)  # slots, current rows, descriptor columns
TABLE_FIELDS = ("ids", "points", "prev_points", "descriptors", "status", "age", "lost", "n_live", "next_id")


@functools.lru_cache(maxsize=None)
def match_table_case(case):
    """(a function that makes the table before the calls, match_index, match_status, cur_uv, cur_desc, cur_count or None, q_count override
    or None, max_lost, with cur_slot)."""
    name, with_count, with_slot = MATCH_TABLE_CASES[case]
    if name != "random":
        table, index, status, k, cur_count, q_count, max_lost = MC.scenario(name)
        uv, desc = MC.cur_rows(k, table.dim)
        return (lambda: MC.scenario(name)[0]), index, status, uv, desc, cur_count, q_count, max_lost, True
    n, k, d = MATCH_TABLE_RANDOM

    def make():
        rng = np.random.default_rng(n * 7 + k)
        live = list(range(0, n, 2))
        table = MC.seeded(n, d, live)
        table.descriptors[live] = rng.standard_normal((len(live), d)).astype(np.float32)
        table.lost[live] = rng.integers(0, 3, len(live))
        return table

    _, _, index, status, uv, desc = MC.random_frame(np.random.default_rng(k), make(), k)
    return make, index, status, uv, desc, (k - 2 if with_count else None), None, 1, with_slot


def match_table_specs(case):
    make, index, status, uv, desc, cur_count, _, _, with_slot = match_table_case(case)
    from feature_tracker_amd import _native as N
    table = make()
    n, d, k = table.n, table.dim, uv.shape[0]
    specs = [_like(name, a) for name, a in table.tensors().items()]
    specs += [_spec("q_uv", (n, 2)), _spec("q_desc", (n, d)), _spec("q_slot", (n,), "int32"), _spec("q_count", (1,), "int32")]
    specs += [_spec("match_index", (n,), "int32"), _spec("match_status", (n,), "uint8"), _spec("cur_uv", (k, 2)), _spec("cur_desc", (k, d))]
    if cur_count is not None:
        specs.append(_spec("cur_count", (1,), "int32"))
    specs.append(_spec("workspace", (-(-N.match_table_workspace_bytes(n, k, d) // 8),), "int64"))  # exactly the declared bytes
    if with_slot:
        specs.append(_spec("cur_slot", (k,), "int32"))
    return specs


def match_query_call(D, ctx, arena):
    a = arena
    D.match_table_query_device(ctx, a["ids"], a["points"], a["descriptors"], a["q_uv"], a["q_desc"], a["q_slot"], a["q_count"])


def match_update_call(D, ctx, arena, max_lost, with_count, with_slot):
    a = arena
    D.match_table_update_device(ctx, a["ids"], a["points"], a["prev_points"], a["descriptors"], a["status"], a["age"], a["lost"], a["n_live"], a["next_id"],
                                a["q_slot"], a["q_count"], a["match_index"], a["match_status"], a["cur_uv"], a["cur_desc"], a["cur_count"] if with_count else None,
                                max_lost, a["workspace"], a["cur_slot"] if with_slot else None)


@pytest.mark.parametrize("case", range(len(MATCH_TABLE_CASES)), ids=[str(c) for c in MATCH_TABLE_CASES])
def test_match_table_on_guarded_memory(ftk, dev_ctx, case):  # noqa: F811
    g = dev_ctx
    make, index, status, uv, desc, cur_count, q_count, max_lost, with_slot = match_table_case(case)
    before, after = make(), make()
    want_query = dict(zip(("q_uv", "q_desc", "q_slot", "q_count"), before.query()))
    q_count_given = want_query["q_count"] if q_count is None else np.array([q_count], np.int32)
    want_slot = after.update(want_query["q_slot"], int(q_count_given[0]), index, status, uv, desc, cur_count, max_lost)
    frame = dict(match_index=index, match_status=status, cur_uv=uv, cur_desc=desc)
    if cur_count is not None:
        frame["cur_count"] = np.array([cur_count], np.int32)
    for fill in FILLS:
        arena = make_arena(match_table_specs(case), dict(before.tensors(), **frame), fill)
        match_query_call(g.D, g.ctx, arena)
        _finish(arena, dict(before.tensors(), **frame))  # the query writes no table tensor
        for name, want in want_query.items():
            assert _same(_np(arena, name), want), (hex(fill), "query", name)
        if q_count is not None:
            arena.put("q_count", q_count_given)  # the scenario's own count, above or below the array
        match_update_call(g.D, g.ctx, arena, max_lost, cur_count is not None, with_slot)
        _finish(arena, dict(frame, q_slot=want_query["q_slot"], q_count=q_count_given))
        for name, want in after.tensors().items():
            assert _same(_np(arena, name), want), (hex(fill), "update", name)
        got_slot = _np(arena, "cur_slot") if with_slot else _np(arena, "workspace").view(np.int32)[:uv.shape[0]]
        assert np.array_equal(got_slot, want_slot), (hex(fill), "cur_slot")


# ---- nn_match_scores_device, nn_match_list_device and nn_fill_pixels_device --------------------------------------------------------------------------
NN_SCORE_SHAPES = [(1, 1), (63, 65), (257, 64), (65, 257)]  # (n_ref, n_cur): tails of the 16-row and the 256-column tile, more than one of each
NN_LIST_SHAPES = [(63, 257), (65, 255), (257, 64)]          # (n_ref, n_cur) across 64 and 256
NN_LIST_ROWS = 40  # fewer than the smallest n_ref: rows without a match stay
NN_MIN_SCORE = -3.0


@functools.lru_cache(maxsize=None)
def nn_scores_case(n_ref, n_cur):
    rng = np.random.default_rng(n_ref * 1000 + n_cur)
    scores = NR.quantised(rng, (1, n_ref, n_cur), nan_rate=0.02)
    idx, st = NR.match_scores(scores, NN_MIN_SCORE)
    return _readonly(scores, idx, st)


def nn_scores_specs(n_ref, n_cur):
    return [_spec("scores", (1, n_ref, n_cur)), _spec("match_index", (1, n_ref), "int32"), _spec("status", (1, n_ref), "uint8")]


def nn_scores_call(D, ctx, arena):
    D.nn_match_scores_device(ctx, arena["scores"], NN_MIN_SCORE, arena["match_index"], arena["status"])


@functools.lru_cache(maxsize=None)
def nn_list_case(n_ref, n_cur):
    """(matches with rows out of range on either side, cur_uv, the restatement's match_index, status and matched_uv)."""
    rng = np.random.default_rng(n_ref * 1000 + n_cur + 1)
    matches = np.stack([rng.integers(-2, n_ref + 3, NN_LIST_ROWS), rng.integers(-2, n_cur + 3, NN_LIST_ROWS)], axis=1).astype(np.int64)
    matches[:4] = [[-1, 0], [n_ref, 0], [0, n_cur], [1, -2]]
    cur_uv = (rng.random((n_cur, 2)) * 300).astype(np.float32)
    idx, st = NR.match_list(matches, n_ref, n_cur)
    return _readonly(matches, cur_uv, idx, st, NR.fill(idx, cur_uv))


def nn_list_specs(n_ref, n_cur):
    return [_spec("matches", (NN_LIST_ROWS, 2), "int64"), _spec("match_index", (n_ref,), "int32"), _spec("status", (n_ref,), "uint8"),
            _spec("cur_uv", (n_cur, 2)), _spec("matched_uv", (n_cur, 2))]


def nn_list_call(D, ctx, arena, n_ref, n_cur):
    D.nn_match_list_device(ctx, arena["matches"], n_ref, n_cur, arena["match_index"], arena["status"])


def nn_fill_call(D, ctx, arena):
    D.nn_fill_pixels_device(ctx, arena["match_index"], arena["cur_uv"], arena["matched_uv"])


@pytest.mark.parametrize("n_ref,n_cur", NN_SCORE_SHAPES)
def test_nn_match_scores_on_guarded_memory(ftk, dev_ctx, n_ref, n_cur):  # noqa: F811
    g = dev_ctx
    scores, idx, st = nn_scores_case(n_ref, n_cur)
    for fill in FILLS:
        arena = make_arena(nn_scores_specs(n_ref, n_cur), dict(scores=scores), fill)
        nn_scores_call(g.D, g.ctx, arena)
        _finish(arena, dict(scores=scores))
        assert np.array_equal(_np(arena, "match_index"), idx) and np.array_equal(_np(arena, "status"), st), hex(fill)


@pytest.mark.parametrize("n_ref,n_cur", NN_LIST_SHAPES)
def test_nn_match_list_and_fill_pixels_on_guarded_memory(ftk, dev_ctx, n_ref, n_cur):  # noqa: F811
    g = dev_ctx
    matches, cur_uv, idx, st, matched = nn_list_case(n_ref, n_cur)
    inputs = dict(matches=matches, cur_uv=cur_uv)
    for fill in FILLS:
        arena = make_arena(nn_list_specs(n_ref, n_cur), inputs, fill)
        nn_list_call(g.D, g.ctx, arena, n_ref, n_cur)
        _finish(arena, inputs)
        assert np.array_equal(_np(arena, "match_index"), idx) and np.array_equal(_np(arena, "status"), st), hex(fill)
        nn_fill_call(g.D, g.ctx, arena)
        _finish(arena, dict(inputs, match_index=idx, status=st))
        assert _same(_np(arena, "matched_uv"), matched), hex(fill)


# ---- dense_flow_device ---------------------------------------------------------------------------------------------------------------------
# (width, height, levels) of tests/test_dense_flow_gpu.py's odd and tiny sizes: the smallest with a partial last tile behind whole ones on both
# axes (at every level), and the smallest with one partial tile on both axes
DENSE_CASES = [(333, 251, 3), (4, 5, 1)]


@functools.lru_cache(maxsize=None)
def dense_case(w, h, levels):
    ref, cur = synth.make_image_pair(max(w, 8), max(h, 8), (1.4, 0.6))
    ref, cur = np.ascontiguousarray(ref[:h, :w]), np.ascontiguousarray(cur[:h, :w])
    rl, cl = synth.build_pyramid(ref, levels), synth.build_pyramid(cur, levels)
    ok, fr, fc, _ = DR.track_pyramid(rl, cl, DR.options())
    assert ok
    inputs = dict(level_inputs("ref", rl), **level_inputs("cur", cl))
    _readonly(fr, fc, *inputs.values())
    return inputs, rl, cl, fr, fc


def dense_specs(w, h, levels):
    _, rl, cl, _, _ = dense_case(w, h, levels)
    return level_specs("ref", rl) + level_specs("cur", cl) + [_spec("flow_r", (h, w)), _spec("flow_c", (h, w))]


def dense_call(F, D, ctx, arena, levels, flow_r=None, flow_c=None):
    D.dense_flow_device(ctx, F.DenseOpticalFlowOptions(), pyramid(D, ctx, arena, "ref", levels), pyramid(D, ctx, arena, "cur", levels),
                        arena["flow_r"] if flow_r is None else flow_r, arena["flow_c"] if flow_c is None else flow_c)


@pytest.mark.parametrize("w,h,levels", DENSE_CASES)
def test_dense_flow_on_guarded_memory(ftk, dev_ctx, w, h, levels):  # noqa: F811
    g, torch = dev_ctx, dev_ctx.torch
    inputs, _, _, want_r, want_c = dense_case(w, h, levels)
    for n, fill in enumerate(FILLS):
        arena = make_arena(dense_specs(w, h, levels), inputs, fill)
        if n == 0:  # one call of the same shape outside the arena makes the context's workspace resident, as the entry's docstring asks
            dense_call(ftk, g.D, g.ctx, arena, levels, torch.empty((h, w), device=g.dev), torch.empty((h, w), device=g.dev))
            _finish(arena, inputs)
        dense_call(ftk, g.D, g.ctx, arena, levels)
        _finish(arena, inputs)
        assert DR.same(_np(arena, "flow_r"), want_r) and DR.same(_np(arena, "flow_c"), want_c), hex(fill)
