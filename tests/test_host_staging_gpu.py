"""The staging of the host-buffer entry points (csrc/ftk_layout.h) on the GPU: every family that has a host-buffer entry and a
*_device entry runs both on the same input, in a fresh context, and the outputs must be bit-identical — both sides launch the same
kernels, the host entry only adds the carve of its staging blocks, the copies and the synchronisation.  The sizes are the smallest
at which a slot that is off by one padding step (256 bytes) overlaps its neighbour: counts just below and above a multiple of 64,
a single element, and descriptor rows that are and are not padded on the way in."""
import ctypes as C

import numpy as np
import pytest

from feature_tracker_amd import _native as N
from feature_tracker_amd import synth
from tests import scenes

pytestmark = pytest.mark.gpu

DEV = "cuda"
WIDTH, HEIGHT, LEVELS = 160, 120, 3
SIZES = (1, 33, 65)


@pytest.fixture(scope="module")
def pair():
    return scenes.scene(WIDTH, HEIGHT, LEVELS)


@pytest.fixture
def fresh():
    """A fresh context on a torch stream of its own (what the device entries' tensors are ordered with), closed afterwards."""
    import torch
    from feature_tracker_amd import device as D

    made = []

    def make():
        stream = torch.cuda.Stream()
        ctx = D.context_on_stream(stream)
        made.append(ctx)
        return torch, D, stream, ctx

    yield make
    for ctx in made:
        ctx.close()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def klt_both(ftk, fresh, pair, n, with_iters):
    """ftk_klt_track and ftk_klt_track_device, basic model, inverse method: (cur_uv, status, iters) of each."""
    torch, D, stream, ctx = fresh()
    opt = ftk.OpticalFlowOptions()
    opt.kMethod = "inverse"
    opt.kMaxTrackPointsNumber = 20000
    ref_uv = scenes.features(n, WIDTH, HEIGHT, half=6)
    rs = np.random.RandomState(n)
    cur_in = (ref_uv + rs.uniform(-1.5, 1.5, ref_uv.shape)).astype(np.float32)  # a prediction that is not the reference position
    st_in = (rs.random_sample(n) < 0.1).astype(np.uint8) * 2                    # some features arrive as already failed
    st_in[0] = 0                                                                # never all of them: the call has work at every n
    with torch.cuda.stream(stream):
        rp, cp = ftk.ImagePyramid.from_host_levels(pair[0], ctx), ftk.ImagePyramid.from_host_levels(pair[1], ctx)
        h_cur, h_st = cur_in.copy(), st_in.copy()
        h_it = np.full(n, 0xFFFFFFFF, np.uint32) if with_iters else None
        native = opt.to_native()
        N.check(N.lib().ftk_klt_track(ctx.handle, N.MODELS["basic"], C.byref(native), rp.handle, cp.handle, _ptr(ref_uv), _ptr(h_cur), _ptr(h_st), n, None, 0, 0,
                                      _ptr(h_it)), ctx.handle)
        d_ref, d_cur, d_st = (torch.from_numpy(x).to(DEV) for x in (ref_uv, cur_in, st_in))
        d_it = torch.full((n,), -1, dtype=torch.int32, device=DEV) if with_iters else None
        D.DeviceKlt("basic", opt, rp, cp, ctx).track(d_ref, d_cur, d_st, d_cur, d_st, iters=d_it)
        stream.synchronize()
        dev = (d_cur.cpu().numpy(), d_st.cpu().numpy(), d_it.cpu().numpy().view(np.uint32) if with_iters else None)
    return (h_cur, h_st, h_it), dev, st_in


def assert_klt_equal(host, dev, st_in, with_iters):
    assert np.array_equal(host[0].view(np.uint32), dev[0].view(np.uint32))  # bit patterns: NaNs included
    assert np.array_equal(host[1], dev[1])
    if with_iters:
        assert np.array_equal(host[2], dev[2])
    assert (host[1] != st_in).any()  # the call did something


@pytest.mark.parametrize("with_iters", (True, False), ids=("iters", "no_iters"))
@pytest.mark.parametrize("n", (1, 63, 65, 257))
def test_klt_track_matches_its_device_entry(ftk, fresh, pair, n, with_iters):
    host, dev, st_in = klt_both(ftk, fresh, pair, n, with_iters)
    assert_klt_equal(host, dev, st_in, with_iters)


def test_klt_track_bulk_copy_branch(ftk, fresh, pair):
    """16 385 features, one past the limit of the zero-copy path: one H2D over (ref_uv, cur_uv, status), one D2H over (cur_uv, status, iters)."""
    host, dev, st_in = klt_both(ftk, fresh, pair, 16385, True)
    assert_klt_equal(host, dev, st_in, True)


def positions(n_ref, n_cur, perm, seed=11):
    rs = np.random.RandomState(seed)
    cur_uv = np.stack([rs.uniform(0, 640, n_cur), rs.uniform(0, 480, n_cur)], axis=1).astype(np.float32)
    pred_uv = np.stack([rs.uniform(0, 640, n_ref), rs.uniform(0, 480, n_ref)], axis=1).astype(np.float32)
    for j, i in enumerate(perm):  # ref i is predicted near cur j where the two are a true pair
        pred_uv[i] = cur_uv[j] + rs.uniform(-30, 30, 2).astype(np.float32)
    return pred_uv, cur_uv


@pytest.mark.parametrize("nearby", (False, True), ids=("force", "nearby"))
@pytest.mark.parametrize("n_bits", (96, 256))
def test_hamming_match_matches_its_device_entry(ftk, fresh, n_bits, nearby):
    """96 bits: 3 words, zero-padded to 4 in the pinned block by the host entry, in a context-owned copy by the device entry."""
    matched = 0
    for n_ref in SIZES:
        for n_cur in SIZES:
            torch, D, stream, ctx = fresh()
            ref, cur, perm = synth.make_descriptors(n_ref, n_cur, n_bits=n_bits, flips=20 if n_bits == 256 else 7)
            thr = 60.0 if n_bits == 256 else 25.0
            pred_uv, cur_uv = positions(n_ref, n_cur, perm) if nearby else (None, None)
            stale = np.arange(n_ref, dtype=np.int32) + 5000  # index_pairs is in/out: entries without a match keep what they held
            m = ftk.BriefMatcher(ctx)
            m.options().kMaxValidDescriptorDistance = thr
            with torch.cuda.stream(stream):
                ok, h_idx = m.NearbyMatch(ref, cur, pred_uv, cur_uv, stale) if nearby else m.ForceMatch(ref, cur, stale)
                assert ok
                d_ref = torch.from_numpy(ftk.pack_brief(ref).view(np.int32)).to(DEV)
                d_cur = torch.from_numpy(ftk.pack_brief(cur).view(np.int32)).to(DEV)
                d_idx = torch.from_numpy(stale).to(DEV)
                kw = dict(pred_uv=torch.from_numpy(pred_uv).to(DEV), cur_uv=torch.from_numpy(cur_uv).to(DEV)) if nearby else {}
                D.hamming_match_device(ctx, d_ref, d_cur, n_bits, thr, d_idx, **kw)
                stream.synchronize()
                assert np.array_equal(h_idx, d_idx.cpu().numpy()), (n_ref, n_cur)
            matched += int((h_idx < 5000).sum())
    assert matched > 20


def test_cosine_force_match_matches_its_device_entry(ftk, fresh):
    matched = 0
    for n_ref in SIZES:
        for n_cur in SIZES:
            torch, D, stream, ctx = fresh()
            ref, cur, _ = synth.make_float_descriptors(n_ref, n_cur, dim=100)  # rows of 400 bytes: no multiple of the slots' alignment
            stale = np.arange(n_ref, dtype=np.int32) + 5000
            m = ftk.CosineMatcher(ctx)
            m.options().kMaxValidDescriptorDistance = 0.3
            with torch.cuda.stream(stream):
                ok, h_idx = m.ForceMatch(ref, cur, stale)
                assert ok
                d_idx = torch.from_numpy(stale).to(DEV)
                D.cosine_match_device(ctx, torch.from_numpy(ref).to(DEV), torch.from_numpy(cur).to(DEV), 0.3, d_idx)
                stream.synchronize()
                assert np.array_equal(h_idx, d_idx.cpu().numpy()), (n_ref, n_cur)
            matched += int((h_idx < 5000).sum())
    assert matched > 20


@pytest.mark.parametrize("n_bits", (96, 256))
def test_brief_compute_matches_its_device_entry(ftk, fresh, pair, n_bits):
    for n in (1, 63, 65, 257):
        torch, D, stream, ctx = fresh()
        uv = scenes.features(n, WIDTH, HEIGHT, half=8)
        b = ftk.BriefDescriptor(ctx)
        b.options().kLength = n_bits
        with torch.cuda.stream(stream):
            pyr = ftk.ImagePyramid.from_host_levels(pair[0][:1], ctx)
            h_words = b.compute_packed(pyr, uv)
            d_words = torch.zeros((n, (n_bits + 31) // 32), dtype=torch.int32, device=DEV)
            D.brief_compute_device(ctx, pyr, torch.from_numpy(uv).to(DEV), n_bits, int(b.options().kHalfPatchSize), d_words)
            stream.synchronize()
            assert np.array_equal(h_words, d_words.cpu().numpy().view(np.uint32)), n
        assert h_words.any()


def test_dense_flow_matches_its_device_entry(ftk, fresh):
    torch, D, stream, ctx = fresh()
    ref, cur = synth.make_image_pair(64, 48, (1.3, -0.8))
    dof = ftk.DenseOpticalFlow(ctx)
    with torch.cuda.stream(stream):
        rp = ftk.ImagePyramid.from_host_levels(synth.build_pyramid(ref, 2), ctx)
        cp = ftk.ImagePyramid.from_host_levels(synth.build_pyramid(cur, 2), ctx)
        ok, (h_r, h_c) = dof.Track(rp, cp)
        assert ok and h_r.shape == (48, 64)
        d_r, d_c = (torch.full((48, 64), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
        D.dense_flow_device(ctx, dof.options(), rp, cp, d_r, d_c)
        stream.synchronize()
        assert np.array_equal(h_r.view(np.uint32), d_r.cpu().numpy().view(np.uint32))
        assert np.array_equal(h_c.view(np.uint32), d_c.cpu().numpy().view(np.uint32))
    assert np.isfinite(h_r).all() and np.abs(h_r).max() > 0.1
