"""The torch device entries (feature_tracker_amd/device.py) off the happy path.

Part A, refusals: for every entry, every tensor argument and every way a torch caller gets it wrong — another dtype, a transposed or
column-sliced view, a buffer one element short, a partner of another width, a host tensor, one of NearbyMatch's two pixel arrays
without the other — the entry raises a ValueError that names the argument, BEFORE the library is called.  Every one of these tests
runs with the native entry points replaced by a stub that records the call, launches nothing and returns an error code, so a missing
check fails as "native call reached" and no bad pointer ever reaches a kernel.

Part B, what must keep working, bit for bit against the oracle: every tensor of a call a view into a larger allocation at a non-zero
offset (with the bytes around every output left alone), int32 and uint32 words, out tensors aliasing in tensors, one-row inputs,
empty inputs, and the caller's remedy for a refused view, ``.contiguous()``.  The views here are misaligned and their tails short; exact
sizes, whole-row overruns and what an output held before the call are tests/test_sparse_entries_guarded_gpu.py's, on 256-byte aligned payloads."""
import types

import numpy as np
import pytest

from feature_tracker_amd import synth
from tests import scenes
from tests.test_direct_method_gpu import CX, CY, FX, FY
from tests.test_direct_method_gpu import scene as direct_scene

pytestmark = pytest.mark.gpu

NATIVE_ENTRIES = ("ftk_klt_track_device", "ftk_klt_track_sharded_device", "ftk_klt_track_shard_device", "ftk_klt_unpack_shards_device",
                  "ftk_hamming_match_device", "ftk_hamming_match_sharded_device", "ftk_cosine_match_device", "ftk_brief_compute_device",
                  "ftk_direct_track_batch_device")


@pytest.fixture
def dev_ctx(ftk):
    import torch
    from feature_tracker_amd import device as D
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    ctx = D.context_on_stream(stream, 0)
    with torch.cuda.stream(stream):
        yield types.SimpleNamespace(torch=torch, D=D, dev=dev, stream=stream, ctx=ctx)
        stream.synchronize()


# ---- part A: refusals ----------------------------------------------------------------------------------------------------------


@pytest.fixture
def native_stub(ftk, monkeypatch):
    """Every device entry point of the loaded library replaced by a recorder that returns FTK_E_INVALID_ARGUMENT and launches nothing."""
    from feature_tracker_amd import _native
    lib = _native.lib()
    calls = []

    def recorder(name):
        def entry(*args):
            calls.append(name)
            return -1
        return entry

    for name in NATIVE_ENTRIES:
        monkeypatch.setattr(lib, name, recorder(name))
    return calls


def _wrong_dtypes(torch, t):
    if t.dtype == torch.float32:
        return [torch.float64]  # torch.from_numpy of a default numpy array
    if t.dtype == torch.uint8:
        return [torch.bool, torch.int32]
    if t.dtype == torch.int64:
        return [torch.int32]
    return [torch.int64]  # int32: torch.full((n,), -1) is int64


def _violations(torch, t, may_shrink):
    """(what, the tensor a careless caller passes instead of ``t``)."""
    for dt in _wrong_dtypes(torch, t):
        yield f"dtype {dt}", t.to(dt)
    if t.dim() == 2:
        n, c = t.shape
        yield "transposed view", torch.zeros((c, n), dtype=t.dtype, device=t.device).t()
        yield "column slice", torch.zeros((n, c + 1), dtype=t.dtype, device=t.device)[:, :c]
    elif t.numel() > 1:
        yield "every other element", torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)[::2]
    if may_shrink:
        yield "one short", t[:-1]
    yield "CPU tensor", t.cpu()


def _refusals(native_stub, call, good, sizing=(), extra=()):
    """Runs ``call(**args)`` once per (argument, violation) and returns what went wrong; ``sizing``: arguments whose length DEFINES a count
    (a shorter one is another valid call or is refused under its partner's name), ``extra``: further (what, argument named, args) cases."""
    import torch
    from feature_tracker_amd._native import FtkError
    cases = []
    for name, t in good.items():
        if t is None:
            continue
        for what, bad in _violations(torch, t, name not in sizing):
            cases.append((f"{name}: {what}", name, dict(good, **{name: bad})))
    cases.extend(extra)
    assert cases
    problems = []
    for what, named, args in cases:
        del native_stub[:]
        message = None
        try:
            call(**args)
            outcome = "accepted"
        except ValueError as e:
            outcome, message = "refused", str(e)
        except FtkError:
            outcome = "passed on to the library"
        if native_stub:
            problems.append(f"{what}: native call reached ({native_stub[0]})")
        elif outcome != "refused":
            problems.append(f"{what}: {outcome}")
        elif named not in message:
            problems.append(f"{what}: the message does not name {named}: {message}")
    return problems


def _klt(ftk, g, n=12):
    ref_levels, cur_levels = scenes.scene(160, 120, 3)
    opt = ftk.OpticalFlowOptions()
    opt.kMethod, opt.kPatchRowHalfSize, opt.kPatchColHalfSize, opt.kMaxTrackPointsNumber = "inverse", 5, 5, n
    klt = g.D.DeviceKlt("basic", opt, g.D.upload_pyramid(ref_levels, g.ctx, g.dev), g.D.upload_pyramid(cur_levels, g.ctx, g.dev), g.ctx)
    t = g.torch
    good = dict(ref_uv=t.full((n, 2), 60.0, device=g.dev), cur_uv_in=t.full((n, 2), 60.0, device=g.dev), status_in=t.zeros(n, dtype=t.uint8, device=g.dev),
                cur_uv_out=t.zeros((n, 2), device=g.dev), status_out=t.zeros(n, dtype=t.uint8, device=g.dev), iters=t.zeros(n, dtype=t.int32, device=g.dev))
    return klt, good


COMM = types.SimpleNamespace(handle=None)  # (never reached: the stub stands in front of the library)


@pytest.mark.parametrize("entry", ["track", "bind", "track_sharded", "bind_sharded"])
def test_klt_entries_refuse_what_the_abi_would_misread(ftk, dev_ctx, native_stub, entry):
    klt, good = _klt(ftk, dev_ctx)
    if entry == "bind_sharded":
        del good["iters"]
    call = {"track": klt.track, "bind": lambda **a: klt.bind(**a)(), "track_sharded": lambda **a: klt.track_sharded(COMM, **a),
            "bind_sharded": lambda **a: klt.bind_sharded(COMM, **a)()}[entry]
    assert _refusals(native_stub, call, good, sizing=("ref_uv",)) == []


def test_klt_shard_halves_refuse_what_the_abi_would_misread(ftk, dev_ctx, native_stub):
    from feature_tracker_amd import _native
    klt, good = _klt(ftk, dev_ctx)
    t, n, world = dev_ctx.torch, 12, 3
    shard = int(_native.lib().ftk_klt_shard_bytes(n, world))
    assert shard == 48  # 4 slots of 9 bytes, rounded up to 16
    args = dict(ref_uv=good["ref_uv"], cur_uv_in=good["cur_uv_in"], status_in=good["status_in"], packed_shard=t.zeros(shard, dtype=t.uint8, device=dev_ctx.dev),
                iters=good["iters"])
    assert _refusals(native_stub, lambda **a: klt.track_shard(1, world, **a), args, sizing=("ref_uv",)) == []
    args = dict(gathered=t.zeros(shard * world, dtype=t.uint8, device=dev_ctx.dev), cur_uv_out=good["cur_uv_out"], status_out=good["status_out"])
    assert _refusals(native_stub, lambda **a: klt.unpack_shards(n=n, world=world, **a), args) == []


def _pairs(g, n_ref, n_cur):
    return dict(pred_uv=g.torch.zeros((n_ref, 2), device=g.dev), cur_uv=g.torch.zeros((n_cur, 2), device=g.dev))


@pytest.mark.parametrize("entry", ["hamming_match_device", "hamming_match_sharded_device"])
def test_hamming_entries_refuse_what_the_abi_would_misread(ftk, dev_ctx, native_stub, entry):
    g, t = dev_ctx, dev_ctx.torch
    n_ref, n_cur, words = 12, 13, 3
    good = dict(ref_words=t.zeros((n_ref, words), dtype=t.int32, device=g.dev), cur_words=t.zeros((n_cur, words), dtype=t.int32, device=g.dev),
                index_pairs=t.full((n_ref,), -1, dtype=t.int32, device=g.dev), **_pairs(g, n_ref, n_cur))
    if entry == "hamming_match_device":
        good["workspace"] = t.zeros(n_ref, dtype=t.int64, device=g.dev)
        call = lambda n_bits=96, **a: g.D.hamming_match_device(g.ctx, a.pop("ref_words"), a.pop("cur_words"), n_bits, 20.0, a.pop("index_pairs"), **a)  # noqa: E731
    else:
        call = lambda n_bits=96, **a: g.D.hamming_match_sharded_device(g.ctx, COMM, a.pop("ref_words"), a.pop("cur_words"), n_bits, 20.0, a.pop("index_pairs"), **a)  # noqa: E731
    extra = [("cur_words narrower than ref_words", "cur_words", dict(good, cur_words=good["cur_words"][:, :2].contiguous())),
             ("ref_words narrower than cur_words", "cur_words", dict(good, ref_words=good["ref_words"][:, :2].contiguous(), n_bits=64)),
             ("n_bits above the width", "n_bits", dict(good, n_bits=97)),
             ("pred_uv without cur_uv", "cur_uv", dict(good, cur_uv=None)),
             ("cur_uv without pred_uv", "pred_uv", dict(good, pred_uv=None))]
    assert _refusals(native_stub, call, good, sizing=("ref_words", "cur_words"), extra=extra) == []


def test_cosine_entry_refuses_what_the_abi_would_misread(ftk, dev_ctx, native_stub):
    g, t = dev_ctx, dev_ctx.torch
    n_ref, n_cur, dim = 12, 13, 16
    good = dict(ref_desc=t.ones((n_ref, dim), device=g.dev), cur_desc=t.ones((n_cur, dim), device=g.dev), index_pairs=t.full((n_ref,), -1, dtype=t.int32, device=g.dev),
                **_pairs(g, n_ref, n_cur))
    call = lambda **a: g.D.cosine_match_device(g.ctx, a.pop("ref_desc"), a.pop("cur_desc"), 0.3, a.pop("index_pairs"), **a)  # noqa: E731
    network_output = t.ones((dim, n_cur), device=g.dev)  # SuperPoint / DISK: [dim, n]
    extra = [("cur_desc narrower than ref_desc", "cur_desc", dict(good, cur_desc=good["cur_desc"][:, :8].contiguous())),
             ("ref_desc narrower than cur_desc", "cur_desc", dict(good, ref_desc=good["ref_desc"][:, :8].contiguous())),
             ("[dim, n] network output as it comes", "cur_desc", dict(good, cur_desc=network_output)),
             ("[dim, n] network output, .t() only", "cur_desc", dict(good, cur_desc=network_output.t())),
             ("pred_uv without cur_uv", "cur_uv", dict(good, cur_uv=None)),
             ("cur_uv without pred_uv", "pred_uv", dict(good, pred_uv=None))]
    assert _refusals(native_stub, call, good, sizing=("ref_desc", "cur_desc"), extra=extra) == []


def test_brief_entry_refuses_what_the_abi_would_misread(ftk, dev_ctx, native_stub):
    g, t = dev_ctx, dev_ctx.torch
    img, _ = synth.make_image_pair(320, 240)
    pyr = g.D.upload_pyramid([img], g.ctx, g.dev)
    n = 12
    good = dict(uv=t.full((n, 2), 100.0, device=g.dev), words_out=t.zeros((n, 3), dtype=t.int32, device=g.dev))
    call = lambda n_bits=96, **a: g.D.brief_compute_device(g.ctx, pyr, a["uv"], n_bits, 8, a["words_out"])  # noqa: E731
    extra = [("words_out one word narrower than n_bits needs", "words_out", dict(good, n_bits=97)),
             ("words_out one word wider than n_bits needs", "words_out", dict(good, n_bits=64)),
             ("[n, 3] points", "uv", dict(good, uv=t.zeros((n, 3), device=g.dev)))]
    assert _refusals(native_stub, call, good, sizing=("uv",), extra=extra) == []


def test_direct_batch_refuses_what_the_abi_would_misread(ftk, dev_ctx, native_stub):
    g, t = dev_ctx, dev_ctx.torch
    rl, cl = scenes.scene(160, 120, 3)
    rp, cp = g.D.upload_pyramid(rl, g.ctx, g.dev), g.D.upload_pyramid(cl, g.ctx, g.dev)
    n = 12

    def tensors():
        return dict(p_c_in_ref=t.ones((n, 3), device=g.dev), ref_uv=t.full((n, 2), 30.0, device=g.dev), cur_uv=t.full((n, 2), 30.0, device=g.dev),
                    pose=t.tensor([1, 0, 0, 0, 0, 0, 0], dtype=t.float32, device=g.dev), status=t.zeros(n, dtype=t.uint8, device=g.dev),
                    iterations=t.zeros(1, dtype=t.int32, device=g.dev))

    first = dict(ref=rp, cur=cp, K=[FX, FY, CX, CY], status_valid=False, **tensors())

    def call(**second):  # the SECOND problem of the batch carries the bad tensor
        g.D.DeviceDirectBatch(ftk.DirectMethodOptions(), [first, dict(ref=rp, cur=cp, K=[FX, FY, CX, CY], status_valid=True, **second)], g.ctx).track()

    assert _refusals(native_stub, call, tensors(), sizing=("ref_uv",)) == []


# ---- part B: what must still work, bit for bit ---------------------------------------------------------------------------------


class Arena:
    """Hands out tensors that are views into larger allocations at chosen element offsets, and afterwards checks that nothing
    outside a view was written."""
    GUARD = 0x5A

    def __init__(self, g):
        self.g, self.held = g, []

    def view(self, values, offset, tail=5):
        torch = self.g.torch
        values = np.ascontiguousarray(values)
        flat = torch.from_numpy(np.frombuffer(bytes([self.GUARD]) * ((values.size + offset + tail) * values.itemsize), dtype=values.dtype).copy()).to(self.g.dev)
        v = flat[offset:offset + values.size].view(values.shape)
        v.copy_(torch.from_numpy(values))
        assert v.data_ptr() == flat.data_ptr() + offset * values.itemsize and v.is_contiguous()
        self.held.append((flat, offset, values.size))
        return v

    def assert_surroundings_untouched(self):
        for flat, offset, size in self.held:
            raw = flat.cpu().numpy().view(np.uint8)
            item = flat.element_size()
            assert (raw[:offset * item] == self.GUARD).all() and (raw[(offset + size) * item:] == self.GUARD).all(), "bytes outside a view were written"


def _positions(n_ref, n_cur, perm, seed=11):
    rs = np.random.RandomState(seed)
    cur_uv = np.stack([rs.uniform(0, 640, n_cur), rs.uniform(0, 480, n_cur)], axis=1).astype(np.float32)
    pred_uv = np.stack([rs.uniform(0, 640, n_ref), rs.uniform(0, 480, n_ref)], axis=1).astype(np.float32)
    for j, i in enumerate(perm):  # ref i is predicted near cur j where the two are a true pair
        if 0 <= i < n_ref:
            pred_uv[i] = cur_uv[j] + rs.uniform(-30, 30, 2).astype(np.float32)
    return pred_uv, cur_uv


N_REF, N_CUR = 130, 257


@pytest.mark.parametrize("nearby", [False, True], ids=["force", "nearby"])
@pytest.mark.parametrize("n_bits", [256, 96])
def test_hamming_on_views_at_offsets_int32_and_uint32(ftk, oracle, dev_ctx, n_bits, nearby):
    """256 bits: 8 words, the MFMA form; 96 bits: 3 words, read at a 12-byte offset and padded to 4 (popcount scan).  Words one ROW into
    their allocation (the offsets a row slice can have), pairs two floats in, index_pairs three elements in; uint32 == int32."""
    g = dev_ctx
    ref, cur, perm = synth.make_descriptors(N_REF, N_CUR, n_bits=n_bits, flips=20 if n_bits == 256 else 7)
    thr = 60.0 if n_bits == 256 else 25.0
    pred_uv, cur_uv = _positions(N_REF, N_CUR, perm)
    stale = np.arange(N_REF, dtype=np.int32) + 5000  # index_pairs is in/out: entries without a match keep what they held
    if nearby:
        ok, want = oracle.nearby_match(ref, cur, pred_uv, cur_uv, thr, 40, 40, stale)
    else:
        ok, want = oracle.force_match(ref, cur, thr, stale)
    assert ok and (want < 5000).sum() > 20
    words = n_bits // 32
    for dtype in (np.int32, np.uint32):
        a = Arena(g)
        d_ref = a.view(ftk.pack_brief(ref).view(dtype), words)
        d_cur = a.view(ftk.pack_brief(cur).view(dtype), words)
        assert d_ref.shape == (N_REF, words) and (d_ref.data_ptr() % 16 != 0) == (n_bits == 96)
        d_idx = a.view(stale, 3)
        kw = dict(pred_uv=a.view(pred_uv, 2), cur_uv=a.view(cur_uv, 2)) if nearby else {}
        g.D.hamming_match_device(g.ctx, d_ref, d_cur, n_bits, thr, d_idx, **kw)
        g.stream.synchronize()
        assert np.array_equal(d_idx.cpu().numpy(), want), dtype
        a.assert_surroundings_untouched()


@pytest.mark.parametrize("small", [None, "0"], ids=["default", "launches"])
@pytest.mark.parametrize("dim", [256, 100])
def test_cosine_on_views_at_offsets(ftk, oracle, dev_ctx, switch, dim, small):
    """Descriptors one float into their allocation (4-byte aligned only), force and nearby; once with the one-launch form switched off."""
    g = dev_ctx
    if small is not None:
        switch("FTK_COSINE_SMALL", small)
    ref, cur, perm = synth.make_float_descriptors(N_REF, N_CUR, dim=dim)
    pred_uv, cur_uv = _positions(N_REF, N_CUR, perm)
    stale = np.arange(N_REF, dtype=np.int32) + 5000
    for nearby in (False, True):
        ok, want = oracle.match_float(ref, cur, 0.3, pred_uv if nearby else None, cur_uv if nearby else None, 40, 40, stale)
        assert ok and (want < 5000).sum() > 20
        a = Arena(g)
        d_ref, d_cur = a.view(ref, 1), a.view(cur, 3)
        assert d_ref.data_ptr() % 16 == 4 and d_cur.data_ptr() % 16 == 12
        d_idx = a.view(stale, 1)
        kw = dict(pred_uv=a.view(pred_uv, 2), cur_uv=a.view(cur_uv, 6)) if nearby else {}
        g.D.cosine_match_device(g.ctx, d_ref, d_cur, 0.3, d_idx, **kw)
        g.stream.synchronize()
        assert np.array_equal(d_idx.cpu().numpy(), want), nearby
        a.assert_surroundings_untouched()


def test_one_row_and_empty_inputs(ftk, oracle, dev_ctx):
    """[1, d] on either side (an extent-1 dimension's stride is arbitrary in torch: ``column.t()`` of a [d, 1] tensor is a legal [1, d]
    row) and n_ref == 0, which every entry accepts and answers by touching nothing."""
    g, t = dev_ctx, dev_ctx.torch
    ref, cur, _ = synth.make_descriptors(N_REF, N_CUR, n_bits=256, flips=20)
    fref, fcur, _ = synth.make_float_descriptors(N_REF, N_CUR, dim=100)
    rw, cw = ftk.pack_brief(ref).view(np.int32), ftk.pack_brief(cur).view(np.int32)
    d_rw, d_cw, d_fr, d_fc = (t.from_numpy(x).to(g.dev) for x in (rw, cw, fref, fcur))
    row = 7919 % N_REF  # cur[1] is ref[row] with flips
    for r0, r1, c0, c1 in ((row, row + 1, 0, N_CUR), (0, N_REF, 1, 2)):
        d_idx = t.full((r1 - r0,), -1, dtype=t.int32, device=g.dev)
        g.D.hamming_match_device(g.ctx, d_rw[r0:r1], d_cw[c0:c1], 256, 60.0, d_idx)
        assert np.array_equal(d_idx.cpu().numpy(), oracle.force_match(ref[r0:r1], cur[c0:c1], 60.0)[1])
        d_idx.fill_(-1)
        g.D.cosine_match_device(g.ctx, d_fr[r0:r1], d_fc[c0:c1], 0.3, d_idx)
        want = oracle.match_float(fref[r0:r1], fcur[c0:c1], 0.3)[1]
        assert np.array_equal(d_idx.cpu().numpy(), want) and (want >= 0).any()
    column = d_fr[row].clone().reshape(100, 1)
    assert column.t().shape == (1, 100) and column.t().stride() == (1, 1)
    d_idx = t.full((1,), -1, dtype=t.int32, device=g.dev)
    g.D.cosine_match_device(g.ctx, column.t(), d_fc, 0.3, d_idx)
    assert np.array_equal(d_idx.cpu().numpy(), oracle.match_float(fref[row:row + 1], fcur, 0.3)[1])
    # empty
    none = t.zeros(0, dtype=t.int32, device=g.dev)
    g.D.hamming_match_device(g.ctx, d_rw[:0], d_cw, 256, 60.0, none)
    g.D.hamming_match_device(g.ctx, d_rw[:0], d_cw, 256, 60.0, none, pred_uv=t.zeros((0, 2), device=g.dev), cur_uv=t.zeros((N_CUR, 2), device=g.dev))
    g.D.cosine_match_device(g.ctx, d_fr[:0], d_fc, 0.3, none)
    d_idx = t.full((N_REF,), 77, dtype=t.int32, device=g.dev)
    g.D.hamming_match_device(g.ctx, d_rw, d_cw[:0], 256, 60.0, d_idx)  # no candidates: index_pairs keeps what it held
    g.D.cosine_match_device(g.ctx, d_fr, d_fc[:0], 0.3, d_idx)
    assert (d_idx.cpu().numpy() == 77).all()
    klt, _ = _klt(ftk, g)
    no_uv, no_st = t.zeros((0, 2), device=g.dev), t.zeros(0, dtype=t.uint8, device=g.dev)
    klt.track(no_uv, no_uv, no_st, no_uv, no_st)
    klt.bind(no_uv, no_uv, no_st, no_uv, no_st, t.zeros(0, dtype=t.int32, device=g.dev))()
    img, _ = synth.make_image_pair(320, 240)
    g.D.brief_compute_device(g.ctx, g.D.upload_pyramid([img], g.ctx, g.dev), no_uv, 256, 8, t.zeros((0, 8), dtype=t.int32, device=g.dev))
    g.stream.synchronize()


def test_the_remedy_for_a_refused_view_is_contiguous(ftk, oracle, dev_ctx):
    """A [dim, n] descriptor matrix (SuperPoint / DISK) and the (u, v) columns of [n, 3] points are refused as views and give the
    oracle's answer on the logical values once the caller passes ``.contiguous()``."""
    g, t = dev_ctx, dev_ctx.torch
    ref, cur, perm = synth.make_float_descriptors(N_REF, N_CUR, dim=100)
    pred_uv, cur_uv = _positions(N_REF, N_CUR, perm)
    net_ref, net_cur = t.from_numpy(np.ascontiguousarray(ref.T)).to(g.dev), t.from_numpy(np.ascontiguousarray(cur.T)).to(g.dev)  # [dim, n]
    pts_ref = t.from_numpy(np.concatenate([pred_uv, np.ones((N_REF, 1), np.float32)], axis=1)).to(g.dev)  # [n, 3]
    pts_cur = t.from_numpy(np.concatenate([cur_uv, np.ones((N_CUR, 1), np.float32)], axis=1)).to(g.dev)
    d_idx = t.full((N_REF,), -1, dtype=t.int32, device=g.dev)
    with pytest.raises(ValueError, match=r"ref_desc.*contiguous\(\)"):
        g.D.cosine_match_device(g.ctx, net_ref.t(), net_cur.t(), 0.3, d_idx)
    with pytest.raises(ValueError, match=r"pred_uv.*contiguous\(\)"):
        g.D.cosine_match_device(g.ctx, net_ref.t().contiguous(), net_cur.t().contiguous(), 0.3, d_idx, pred_uv=pts_ref[:, :2], cur_uv=pts_cur[:, :2])
    assert (d_idx.cpu().numpy() == -1).all()
    g.D.cosine_match_device(g.ctx, net_ref.t().contiguous(), net_cur.t().contiguous(), 0.3, d_idx, pred_uv=pts_ref[:, :2].contiguous(),
                            cur_uv=pts_cur[:, :2].contiguous())
    want = oracle.match_float(ref, cur, 0.3, pred_uv, cur_uv)[1]
    assert np.array_equal(d_idx.cpu().numpy(), want) and (want >= 0).sum() > 20
    # the same columns in front of BRIEF
    img, _ = synth.make_image_pair(320, 240)
    uv = scenes.features(64, 320, 240, half=8)
    pts = t.from_numpy(np.concatenate([uv, np.ones((64, 1), np.float32)], axis=1)).to(g.dev)
    pyr = g.D.upload_pyramid([img], g.ctx, g.dev)
    words = t.zeros((64, 8), dtype=t.int32, device=g.dev)
    with pytest.raises(ValueError, match=r"uv.*contiguous\(\)"):
        g.D.brief_compute_device(g.ctx, pyr, pts[:, :2], 256, 8, words)
    g.D.brief_compute_device(g.ctx, pyr, pts[:, :2].contiguous(), 256, 8, words)
    assert np.array_equal(words.cpu().numpy().view(np.uint32), ftk.pack_brief(oracle.brief_compute(img, uv, 256, 8)[1]))


def test_brief_on_views_at_offsets(ftk, oracle, dev_ctx):
    g = dev_ctx
    img, _ = synth.make_image_pair(320, 240)
    uv = scenes.features(64, 320, 240, half=8)
    ok, bits = oracle.brief_compute(img, uv, 256, 8)
    assert ok and bits.any(axis=1).sum() > 40
    pyr = g.D.upload_pyramid([img], g.ctx, g.dev)
    for dtype in (np.int32, np.uint32):
        a = Arena(g)
        d_uv, d_words = a.view(uv, 2), a.view(np.zeros((64, 8), dtype), 8)
        g.D.brief_compute_device(g.ctx, pyr, d_uv, 256, 8, d_words)
        g.stream.synchronize()
        assert np.array_equal(d_words.cpu().numpy().view(np.uint32), ftk.pack_brief(bits)), dtype
        a.assert_surroundings_untouched()


KLT_VARIANTS = [("basic", "inverse"), ("affine", "inverse"), ("lssd", "fast")]


def _klt_case(ftk, oracle, g, model, method, n=64):
    ref_levels, cur_levels = scenes.scene(160, 120, 3)
    uv = scenes.features(n, 160, 120, half=5)
    status = (np.arange(n) % 9 == 4).astype(np.uint8) * 3  # some features arrive as kOutside and are passed through
    opt = ftk.OpticalFlowOptions()
    opt.kMethod, opt.kPatchRowHalfSize, opt.kPatchColHalfSize, opt.kMaxTrackPointsNumber = method, 5, 5, n
    klt = g.D.DeviceKlt(model, opt, g.D.upload_pyramid(ref_levels, g.ctx, g.dev), g.D.upload_pyramid(cur_levels, g.ctx, g.dev), g.ctx)
    ok, c, s, it = oracle.klt_track_pyramid(model, ref_levels, cur_levels, uv, uv, status, method=method, half=5, max_points=n)
    assert ok and (s == 1).sum() > n // 2
    return klt, uv, status, c, s, it


@pytest.mark.parametrize("model,method", KLT_VARIANTS)
def test_klt_on_views_at_offsets(ftk, oracle, dev_ctx, model, method):
    """Pairs two floats into their allocation (8-byte aligned, not 16), status and iteration counts at odd element offsets."""
    g = dev_ctx
    klt, uv, status, c, s, it = _klt_case(ftk, oracle, g, model, method)
    n = len(uv)
    for how in ("track", "bind"):
        a = Arena(g)
        d_ref, d_in, d_st = a.view(uv, 2), a.view(uv, 6), a.view(status, 3)
        d_out, d_so, d_it = a.view(np.zeros((n, 2), np.float32), 2), a.view(np.zeros(n, np.uint8), 1), a.view(np.zeros(n, np.int32), 3)
        assert d_ref.data_ptr() % 16 == 8
        if how == "track":
            klt.track(d_ref, d_in, d_st, d_out, d_so, d_it)
        else:
            klt.bind(d_ref, d_in, d_st, d_out, d_so, d_it)()
        g.stream.synchronize()
        assert np.array_equal(d_so.cpu().numpy(), s), how
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), c.view(np.uint32)), how
        assert np.array_equal(d_it.cpu().numpy().astype(np.uint32), np.asarray(it, np.uint32)), how
        a.assert_surroundings_untouched()


@pytest.mark.parametrize("model,method", KLT_VARIANTS)
def test_klt_out_tensors_aliasing_in_tensors(ftk, oracle, dev_ctx, model, method):
    """cur_uv_out is cur_uv_in and status_out is status_in (in place, as the reference), through ``track`` and through ``bind``."""
    g, t = dev_ctx, dev_ctx.torch
    klt, uv, status, c, s, _ = _klt_case(ftk, oracle, g, model, method)
    d_ref = t.from_numpy(uv).to(g.dev)
    for how in ("track", "bind"):
        d_pos, d_st = t.from_numpy(uv.copy()).to(g.dev), t.from_numpy(status.copy()).to(g.dev)
        if how == "track":
            klt.track(d_ref, d_pos, d_st, d_pos, d_st)
        else:
            klt.bind(d_ref, d_pos, d_st, d_pos, d_st)()
        g.stream.synchronize()
        assert np.array_equal(d_st.cpu().numpy(), s), how
        assert np.array_equal(d_pos.cpu().numpy().view(np.uint32), c.view(np.uint32)), how


def test_direct_batch_on_views_at_offsets(ftk, oracle, dev_ctx):
    """Two problems of 30 points; every tensor of both a view at a non-zero offset (points and pairs one row in, pose one float in, status
    three bytes in, the iteration count one element in)."""
    g = dev_ctx
    rl, cl, uv_all, pts_all = direct_scene(w=320, h=240, levels=3, n=31)
    rp, cp = g.D.upload_pyramid(rl, g.ctx, g.dev), g.D.upload_pyramid(cl, g.ctx, g.dev)
    a, problems, host = Arena(g), [], []
    for k in range(2):
        uv, pts = np.ascontiguousarray(uv_all[k:k + 30]), np.ascontiguousarray(pts_all[k:k + 30])
        host.append((uv, pts))
        problems.append(dict(ref=rp, cur=cp, K=[FX, FY, CX, CY], p_c_in_ref=a.view(pts, 3), ref_uv=a.view(uv, 2), cur_uv=a.view(uv, 2),
                             pose=a.view(np.float32([1, 0, 0, 0, 0, 0, 0]), 1), status=a.view(np.zeros(30, np.uint8), 3), status_valid=False,
                             iterations=a.view(np.zeros(1, np.int32), 1)))
    g.D.DeviceDirectBatch(ftk.DirectMethodOptions(), problems, g.ctx).track()
    g.stream.synchronize()
    for (uv, pts), pr in zip(host, problems):
        ok, c, q, p, st, it = oracle.direct_track(rl, cl, [FX, FY, CX, CY], pts, uv)
        pose = pr["pose"].cpu().numpy()
        assert ok and it > 0
        assert np.array_equal(pose[:4].view(np.uint32), np.float32(q).view(np.uint32)) and np.array_equal(pose[4:].view(np.uint32), np.float32(p).view(np.uint32))
        assert np.array_equal(pr["cur_uv"].cpu().numpy().view(np.uint32), c.view(np.uint32))
        assert np.array_equal(pr["status"].cpu().numpy(), st)
        assert int(pr["iterations"].cpu().numpy()[0]) == it
    a.assert_surroundings_untouched()
