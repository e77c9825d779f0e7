"""The four device entries that take a workspace from the caller, held to the sizes they declare:
``epipolar_ransac_device``, ``two_view_ransac_device``, ``keypoint_decode_device`` and ``match_assignment_device`` called directly, not
through the classes (which may give a workspace room to spare), on guarded memory (tests/guarded.py):

 (a) the workspace holds exactly ``ceil(*_workspace_bytes / 8)`` int64 words, nothing more;
 (b) every output is a guarded payload of exactly its documented shape, the optional ones present in one run and absent in another;
 (c) every call is made twice on fresh arenas, all payloads 0x00 and all payloads 0xFF (NaN floats, -1 counts, all-ones keys), and both
     results equal the scalar restatement bit for bit: nothing depends on what the workspace or an output held before;
 (d) no guard band is written;
 (e) the inputs, guarded payloads too, come back bit for bit.

Every payload starts 256-byte aligned, as a block of torch's allocator does, so the entries see the alignment they see from their usual
callers (the vector path of MatchAssignment included).  No kernel is run out of bounds here: the one damaged guard of this file is
written by a torch indexing op."""
import functools

import numpy as np
import pytest

from tests import epipolar_ref as E
from tests import guarded as G
from tests import keypoint_decode_ref as KD
from tests import match_assignment_ref as MA
from tests import two_view_ref as T

pytestmark = pytest.mark.gpu

FILLS = (G.ZEROS, G.ONES)


def _words(nbytes):
    """(a): the workspace's int64 elements for a declared byte count, with no added term."""
    return -(-int(nbytes) // 8)


def _ctx(ftk):
    return ftk.default_context()


def _finish(arena, inputs):
    """(d) and (e) after the call: one synchronisation, one copy of the arena, every guard intact, every input as it was."""
    import torch
    torch.cuda.synchronize()
    host = arena.check()
    for name, array in inputs.items():
        assert arena.payload_bytes(name, host).tobytes() == np.ascontiguousarray(array).tobytes(), f"the call changed its input {name}"
    return host


def _np(arena, name):
    return arena[name].cpu().numpy()


# ---- the helper itself, on the device -----------------------------------------------------------------------------------------------------

def test_the_guards_notice_one_element_past_a_payload_on_the_device(ftk):
    import torch
    specs = [("ref_uv", "float32", (257, 2), 0), ("workspace", "int64", (1031,), 0), ("counts", "int32", (65,), 0)]
    for arena in G.poison_pair(specs, "cuda"):
        assert arena.buf.is_cuda and arena["workspace"].data_ptr() % G.ALIGN == 0
        arena.check()
    arena = G.Arena(specs, "cuda", fill=G.ONES)
    a, b = arena.span("workspace")
    longer = arena.buf[a:b + 8].view(torch.int64)  # the payload and one element of the guard behind it
    longer[torch.tensor([1031], device="cuda")] = 7
    with pytest.raises(G.GuardDamaged) as e:
        arena.check()
    assert (e.value.before, e.value.after, e.value.first, e.value.past_before) == ("workspace", "counts", b, 0)
    assert (arena["workspace"] == -1).all()


# ---- epipolar_ransac_device ---------------------------------------------------------------------------------------------------------------

def _epipolar_run(ftk, ref, cur, status, image, threshold, K, seed, fill, with_hypotheses):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    n = len(ref)
    specs = [("ref_uv", "float32", (n, 2), 0), ("cur_uv", "float32", (n, 2), 0), ("status", "uint8", (n,), 0),
             ("workspace", "int64", (_words(N.epipolar_workspace_bytes(n, K)),), 0), ("best", "int32", (1,), 0), ("n_inliers", "int32", (1,), 0),
             ("F", "float32", (3, 3), 0)]
    if with_hypotheses:
        specs += [("counts", "int32", (K,), 0), ("models", "float32", (K, 9), 0)]
    arena = G.Arena(specs, "cuda", fill=fill)
    inputs = dict(ref_uv=ref, cur_uv=cur)
    for name, array in dict(inputs, status=status).items():
        arena.put(name, array)
    D.epipolar_ransac_device(_ctx(ftk), arena["ref_uv"], arena["cur_uv"], arena["status"], image, threshold, K, seed, arena["workspace"], arena["best"],
                             arena["n_inliers"], arena["F"], arena["counts"] if with_hypotheses else None, arena["models"] if with_hypotheses else None)
    _finish(arena, inputs)
    return arena


def _epipolar_equal(arena, want, with_hypotheses, what):
    for field in ("status", "F") + (("counts", "models") if with_hypotheses else ()):
        assert E.same(_np(arena, field), getattr(want, field)), (what, field)
    assert (int(_np(arena, "best")[0]), int(_np(arena, "n_inliers")[0])) == (want.best, want.n_inliers), what


def _epipolar_case(ftk, name, threshold, K, seed):
    ref, cur, status, image = E.case(name)
    want = E.ransac(ref, cur, status, image, threshold, K, seed)
    for fill in FILLS:
        for with_hypotheses in (True, False):
            arena = _epipolar_run(ftk, ref, cur, status, image, threshold, K, seed, fill, with_hypotheses)
            _epipolar_equal(arena, want, with_hypotheses, (name, K, hex(fill), with_hypotheses))
    return want


@pytest.mark.parametrize("K", [1, 63, 65])
@pytest.mark.parametrize("name", ["n7", "n8", "n9", "n64_half", "n257", "n1025"])
def test_epipolar_ransac_in_its_declared_bytes(ftk, name, K):
    want = _epipolar_case(ftk, name, 1.0, K, 3)
    if name == "n7":  # M < 8: nothing is formed, every hypothesis is invalid
        assert (want.best, want.n_inliers) == (-1, 7) and (want.counts == -1).all()


def test_epipolar_ransac_in_its_declared_bytes_on_hostile_points(ftk):
    for threshold in (1.0, 0.0):
        _epipolar_case(ftk, "hostile", threshold, 64, 0)


# ---- two_view_ransac_device ---------------------------------------------------------------------------------------------------------------

def _two_view_run(ftk, ref, cur, status, image, threshold, K, seed, mode, fill, with_hypotheses, permille=750):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    n = len(ref)
    specs = [("ref_uv", "float32", (n, 2), 0), ("cur_uv", "float32", (n, 2), 0), ("status", "uint8", (n,), 0),
             ("workspace", "int64", (_words(N.two_view_workspace_bytes(n, K, N.TWO_VIEW_MODES[mode])),), 0), ("model", "int32", (1,), 0),
             ("best", "int32", (2,), 0), ("n_inliers", "int32", (2,), 0), ("F", "float32", (3, 3), 0), ("H", "float32", (3, 3), 0)]
    if with_hypotheses:
        specs += [("counts", "int32", (2, K), 0), ("models", "float32", (2, K, 9), 0)]
    arena = G.Arena(specs, "cuda", fill=fill)
    inputs = dict(ref_uv=ref, cur_uv=cur)
    for name, array in dict(inputs, status=status).items():
        arena.put(name, array)
    D.two_view_ransac_device(_ctx(ftk), arena["ref_uv"], arena["cur_uv"], arena["status"], image, threshold, K, seed, mode, permille, arena["workspace"],
                             arena["model"], arena["best"], arena["n_inliers"], arena["F"], arena["H"], arena["counts"] if with_hypotheses else None,
                             arena["models"] if with_hypotheses else None)
    _finish(arena, inputs)
    return arena


def _two_view_equal(arena, want, with_hypotheses, what):
    got = T.Result()
    got.model = int(_np(arena, "model")[0])
    for field in T.OUTPUTS:
        # without counts and models the call has no such outputs: what is left to compare is every other one
        setattr(got, field, _np(arena, field) if with_hypotheses or field not in ("counts", "models") else getattr(want, field))
    assert T.same_results(got, want) == [], what
    return got


@pytest.mark.parametrize("mode", ["fundamental", "homography", "auto"])
@pytest.mark.parametrize("K", [1, 65])
@pytest.mark.parametrize("name", ["n3", "n4", "n5", "n8", "n9", "n257", "plane300"])
def test_two_view_ransac_in_its_declared_bytes(ftk, name, K, mode):
    ref, cur, status, image = T.case(name)
    want = T.ransac(ref, cur, status, image, 1.0, K, 3, mode)
    for fill in FILLS:
        for with_hypotheses in (True, False):
            arena = _two_view_run(ftk, ref, cur, status, image, 1.0, K, 3, mode, fill, with_hypotheses)
            got = _two_view_equal(arena, want, with_hypotheses, (name, K, mode, hex(fill), with_hypotheses))
            idle = {"fundamental": 1, "homography": 0}.get(mode)
            if idle is not None:  # the slot of the model that did not run: no hypothesis, whatever the memory held
                assert got.best[idle] == -1 and not (got.H if idle else got.F).view(np.uint32).any(), (name, K, mode, hex(fill))
                if with_hypotheses:
                    assert (got.counts[idle] == -1).all() and not got.models[idle].view(np.uint32).any(), (name, K, mode, hex(fill))


# ---- keypoint_decode_device ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _survivors(name):
    semi, desc, kw = KD.case(name)
    return KD.decode(semi, desc, max_keypoints=4096, **kw).survivors


def _keypoint_run(ftk, semi, desc, K, kw, layout, fill, with_heatmap):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    _, hc, wc = semi.shape
    d = desc.shape[0]
    mem = np.ascontiguousarray(desc) if layout == "chw" else np.ascontiguousarray(np.transpose(desc, (1, 2, 0)))
    occupied, mask = kw.get("occupied"), kw.get("occupied_mask")
    n_occ = 0 if occupied is None else len(occupied)
    nbytes = N.keypoint_decode_workspace_bytes(hc, wc, kw["min_distance"], n_occ)
    specs = [("semi", "float32", semi.shape, 0), ("desc", "float32", mem.shape, 0)]
    inputs = dict(semi=semi, desc=mem)
    if occupied is not None:
        specs.append(("occupied", "float32", (n_occ, 2), 0))
        inputs["occupied"] = occupied
        if mask is not None:
            specs.append(("occupied_mask", "uint8", (n_occ,), 0))
            inputs["occupied_mask"] = mask
    # the workspace last but for the outputs: with no occupied points the band behind it is where a stamp plane would lie
    specs += [("workspace", "int64", (_words(nbytes),), 0), ("uv", "float32", (K, 2), 0), ("scores", "float32", (K,), 0),
              ("descriptors", "float32", (K, d), 0), ("count", "int32", (1,), 0)]
    if with_heatmap:
        specs.append(("heatmap", "float32", (8 * hc, 8 * wc), 0))
    arena = G.Arena(specs, "cuda", fill=fill)
    for name, array in inputs.items():
        arena.put(name, array)
    D.keypoint_decode_device(_ctx(ftk), arena["semi"], arena["desc"], K, kw["min_score"], kw["min_distance"], kw["border"], arena["workspace"], arena["uv"],
                             arena["scores"], arena["descriptors"], arena["count"], arena["heatmap"] if with_heatmap else None,
                             arena["occupied"] if occupied is not None else None, arena["occupied_mask"] if mask is not None else None, layout)
    _finish(arena, inputs)
    return arena


def _keypoint_equal(arena, want, with_heatmap, what):
    got = KD.Result()
    got.uv, got.scores, got.descriptors, got.count = _np(arena, "uv"), _np(arena, "scores"), _np(arena, "descriptors"), int(_np(arena, "count")[0])
    got.heatmap = _np(arena, "heatmap") if with_heatmap else want.heatmap  # (no such output in this run)
    assert KD.same_results(got, want) == [], what
    # the rows behind count are zeros: every bit
    for field in ("uv", "scores", "descriptors"):
        assert not getattr(got, field)[got.count:].view(np.uint32).any(), (what, field)
    return got


@pytest.mark.parametrize("name", list(KD.CASES))
def test_keypoint_decode_in_its_declared_bytes(ftk, name):
    from feature_tracker_amd import _native as N
    semi, desc, kw = KD.case(name)
    S = _survivors(name)
    assert S >= 2
    hc, wc = semi.shape[1:]
    if "occupied" not in kw:  # the declared bytes hold no stamp planes
        assert N.keypoint_decode_workspace_bytes(hc, wc, kw["min_distance"], 0) + 2 * ((64 * hc * wc + 15) & ~15) == \
            N.keypoint_decode_workspace_bytes(hc, wc, kw["min_distance"], 1)
    for K in (S - 1, S, S + 3):
        want = KD.decode(semi, desc, max_keypoints=K, **kw)
        assert want.count == min(S, K)
        for layout in KD.LAYOUTS:
            for fill in FILLS:
                for with_heatmap in (True, False):
                    arena = _keypoint_run(ftk, semi, desc, K, kw, layout, fill, with_heatmap)
                    _keypoint_equal(arena, want, with_heatmap, (name, K, layout, hex(fill), with_heatmap))


# ---- match_assignment_device --------------------------------------------------------------------------------------------------------------

MA_IDS = ["x".join(str(v) for v in s[:3]) for s in MA.SHAPES]


def _padded(n):
    """A row stride above N + 1 that keeps every row 16-byte aligned."""
    return (n + 1 + 3) // 4 * 4 + 4


def _match_run(ftk, a, b, kw, counts, stride, fill):
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    (m, d), n = a.shape, b.shape[0]
    weights, bias = kw.get("weights"), kw.get("bias")
    row_stride = n + 1 if stride is None else stride
    specs = [("desc0", "float32", (m, d), 0), ("desc1", "float32", (n, d), 0)]
    inputs = dict(desc0=a, desc1=b)
    if weights is not None:
        specs += [("weights", "float32", (d + 1, d), 0), ("bias", "float32", (d + 1,), 0)]
        inputs.update(weights=weights, bias=bias)
    if counts is not None:
        specs += [("count0", "int32", (1,), 0), ("count1", "int32", (1,), 0)]
        inputs.update(count0=np.array([counts[0]], np.int32), count1=np.array([counts[1]], np.int32))
    specs += [("workspace", "int64", (_words(N.match_assignment_workspace_bytes(m, n, d, weights is not None)),), 0),
              ("scores", "float32", (m * row_stride + n + 1,), 0)]
    arena = G.Arena(specs, "cuda", fill=fill)
    for name, array in inputs.items():
        arena.put(name, array)
    D.match_assignment_device(_ctx(ftk), arena["desc0"], arena["desc1"], arena["weights"] if weights is not None else None,
                              arena["bias"] if weights is not None else None, None if weights is not None else MA.default_scale(d),
                              arena["count0"] if counts is not None else None, arena["count1"] if counts is not None else None, arena["workspace"],
                              arena["scores"], stride)
    _finish(arena, inputs)
    return arena


def _match_equal(arena, want, m, n, row_stride, fill, what):
    flat = _np(arena, "scores")
    assert flat.shape == (m * row_stride + n + 1,)
    rows = np.zeros((m + 1, row_stride), np.float32)
    rows.view(np.uint8)[:] = fill
    rows.reshape(-1)[:flat.size] = flat
    assert MA.same(rows[:, :n + 1], want), what
    # the padding behind the first N + 1 floats of the rows that have one keeps every byte of its fill
    assert (rows[:m, n + 1:].view(np.uint8) == fill).all(), what


@pytest.mark.parametrize("with_weights", [False, True], ids=["without_weights", "with_weights"])
@pytest.mark.parametrize("shape", MA.SHAPES, ids=MA_IDS)
def test_match_assignment_in_its_declared_bytes(ftk, shape, with_weights):
    a, b, kw = MA.case(shape, with_weights)
    m, n = shape[:2]
    given = ((2 * m + 2) // 3, (3 * n + 3) // 4)  # some rows and columns invalid (none where there is only one)
    for counts in (None, given):
        want = MA.assign(a, b, **kw) if counts is None else MA.assign(a, b, count0=counts[0], count1=counts[1], **kw)
        for stride in (None, n + 1, _padded(n)):
            for fill in FILLS:
                arena = _match_run(ftk, a, b, kw, counts, stride, fill)
                _match_equal(arena, want, m, n, n + 1 if stride is None else stride, fill, (shape, with_weights, counts, stride, hex(fill)))
