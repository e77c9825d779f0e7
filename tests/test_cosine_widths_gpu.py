"""GPU parity tests: the cosine matcher at EVERY descriptor width, indices bit for bit against oracle.match_float (as in
tests/test_float_matcher_gpu.py, which stops at 256 components and so at three of the kernel's instantiations).

tests/cosine_width_cases.py names the widths and builds the inputs; tests/test_cosine_widths_cpu.py shows on the CPU which form every
width plans (register-stationary with 4 / 8 / 12 / 16 K steps, the chunked pair with 5 .. 64 chunks, either prep kernel), that the
widths take every branch of the exact dot product, that the inputs are what they claim to be, that the oracle agrees with float64
at these widths and that the comparison notices a mutant."""
import functools

import numpy as np
import pytest

from tests import cosine_width_cases as W

pytestmark = pytest.mark.gpu

COL, ROW = W.WINDOW


def matcher(ftk, max_dist, col=COL, row=ROW):
    m = ftk.CosineMatcher()
    m.options().kMaxValidDescriptorDistance = max_dist
    m.options().kMaxValidPredictColDistance = col
    m.options().kMaxValidPredictRowDistance = row
    return m


@functools.lru_cache(maxsize=None)
def expected(builder, *args):
    """(case, {("force", thr) | ("nearby", thr): oracle indices}) of a builder of cosine_width_cases, computed once and frozen."""
    from tests import oracle_lib
    oracle_lib.lib()
    c = getattr(W, builder)(*args)
    want = {}
    with np.errstate(all="ignore"):
        for thr in W.FORCE_THRESHOLDS:
            want["force", thr] = oracle_lib.match_float(c.ref, c.cur, thr)[1]
        want["nearby", W.NEARBY_THRESHOLD] = oracle_lib.match_float(c.ref, c.cur, W.NEARBY_THRESHOLD, c.pred_uv, c.cur_uv, max_col=COL, max_row=ROW)[1]
    for v in want.values():
        v.setflags(write=False)
    return c, want


def run(ftk, builder, *args, what=()):
    c, want = expected(builder, *args)
    for (form, thr), idx_c in want.items():
        with np.errstate(all="ignore"):
            if form == "force":
                ok, idx_g = matcher(ftk, thr).ForceMatch(c.ref, c.cur)
            else:
                ok, idx_g = matcher(ftk, thr).NearbyMatch(c.ref, c.cur, c.pred_uv, c.cur_uv)
        assert ok is True
        assert np.array_equal(idx_g, idx_c), (builder, args, what, form, thr, np.flatnonzero(idx_g != idx_c)[:10], idx_g[idx_g != idx_c][:10], idx_c[idx_g != idx_c][:10])
    return want


@pytest.mark.parametrize("dim", W.WIDTHS)
def test_every_width_force_and_nearby(ftk, switch, dim):
    """planted and near_ties, ForceMatch at 0.1 and 0.6 and NearbyMatch at 0.9, under the default dispatch; 64, 128 and 256 (one launch
    by default at this size) also through the launches that serve the large calls."""
    for small in (None, "0") if dim in (64, 128, 256) else (None,):
        switch("FTK_COSINE_SMALL", small)
        for builder in ("planted", "near_ties"):
            want = run(ftk, builder, dim, what=("small", small))
            assert any((idx >= 0).any() for idx in want.values())


@pytest.mark.parametrize("splits", ["1", "2", "5"])
@pytest.mark.parametrize("dim", [160, 192, 320, 1000, 4096])
def test_wide_forms_at_forced_splits(ftk, switch, dim, splits):
    """The 12-step register-stationary kernel and the chunked pair at 5, 16 and 64 chunks with one, two and (capped by the tiles) five
    workgroups per row group; 160 and 192 also through the chunked pair, which then runs 3 chunks."""
    switch("FTK_COSINE_SPLITS", splits)
    for chunked in (None, "1") if dim <= 192 else (None,):
        switch("FTK_COSINE_CHUNKED", chunked)
        for builder in ("planted", "near_ties"):
            run(ftk, builder, dim, what=("splits", splits, "chunked", chunked))


@pytest.mark.parametrize("dim", [512, 1000, 2048, 4096])
def test_heavy_tailed_rows_keep_the_deciding_pair(ftk, dim):
    """Rows whose components are fp16 subnormals but for 8, with a near-tie group on them: force and nearby."""
    want = run(ftk, "heavy_tail", dim)
    assert (want["force", 0.6][list(W.TIE_ROWS)] >= 0).all()


@pytest.mark.parametrize("dim", [160, 320, 4096])
def test_irregular_rows_and_overflow_at_wide_widths(ftk, dim):
    """Zero, NaN, inf, overflowing and underflowing rows (a few, then more than the side list holds), and a candidate list that
    overflows on every row: the exact scan over all candidates at 3, 5 and 64 chunks' width."""
    run(ftk, "irregular", dim)
    run(ftk, "irregular", dim, True)
    want = run(ftk, "overflow", dim)
    assert (want["force", 0.6] < 12).all() and (want["force", 0.6] >= 0).any()  # the lowest index of each group of copies


@pytest.mark.parametrize("dim", [160, 1024])
def test_zero_distance_stop_at_wide_widths(ftk, oracle, dim):
    """The construction of test_nearby_scan_stops_at_the_first_exact_zero_distance (tests/test_float_matcher_gpu.py): scaled copies of
    the reference row at distance exactly 0 and below 0, in every order; NearbyMatch stops at the first zero, ForceMatch does not."""
    rs = np.random.RandomState(dim)
    n_ref, n_cur = 32, 400
    ref = rs.standard_normal((n_ref, dim)).astype(np.float32)
    cur = rs.standard_normal((n_cur, dim)).astype(np.float32)
    cases = 0
    for i in range(n_ref):
        zero, neg = [], []
        for k in range(300):
            s = np.float32(0.5 + k * 0.0037)
            d = oracle.cosine_distance(ref[i], (ref[i] * s).astype(np.float32))
            (zero if d == 0 else neg if d < 0 else []).append(s)
        if not zero or not neg:
            continue
        cases += 1
        slots = np.sort(rs.choice(n_cur, size=4, replace=False))
        order = [(zero, neg, neg, zero), (neg, zero, neg, zero), (zero, zero, neg, neg), (neg, neg, zero, neg)][i % 4]
        for slot, pool in zip(slots, order):
            cur[slot] = ref[i] * pool[rs.randint(len(pool))]
    assert cases > n_ref // 2
    uv = np.zeros((n_ref, 2), np.float32)
    cuv = np.zeros((n_cur, 2), np.float32)  # every candidate inside every window
    for thr in (0.05, 0.6):
        ok_g, idx_g = matcher(ftk, thr).NearbyMatch(ref, cur, uv, cuv)
        ok_c, idx_c = oracle.match_float(ref, cur, thr, uv, cuv)
        assert ok_g and ok_c and np.array_equal(idx_g, idx_c), np.flatnonzero(idx_g != idx_c)[:10]
        okf, idx_f = matcher(ftk, thr).ForceMatch(ref, cur)
        okc, idx_fc = oracle.match_float(ref, cur, thr)
        assert np.array_equal(idx_f, idx_fc)
    assert (idx_g != idx_f).any()  # the stop changes the answer for some rows, so the case is exercised


@pytest.mark.parametrize("dim", [136, 192, 264, 4096])
def test_unaligned_device_buffers_at_wide_widths(ftk, oracle, dim):
    """Widths that are multiples of 8 take the packet-wide prep only from 16-byte aligned rows: views 12 and 4 bytes into a larger
    tensor send them through the octet prep (test_device_buffers_not_16_byte_aligned at 12 K steps, 5 and 64 chunks)."""
    import torch
    from feature_tracker_amd import device as D
    c, want = expected("near_ties", dim)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        ctx = D.context_on_stream(stream, 0)
        big_r = torch.zeros(c.ref.size + 3, dtype=torch.float32, device=dev)
        big_c = torch.zeros(c.cur.size + 1, dtype=torch.float32, device=dev)
        d_ref = big_r[3:].view(c.ref.shape)   # base + 12 bytes
        d_cur = big_c[1:].view(c.cur.shape)   # base + 4 bytes
        d_ref.copy_(torch.from_numpy(c.ref.copy()))
        d_cur.copy_(torch.from_numpy(c.cur.copy()))
        assert d_ref.data_ptr() % 16 != 0 and d_cur.data_ptr() % 16 != 0
        for thr in W.FORCE_THRESHOLDS:
            idx = torch.full((c.ref.shape[0],), -1, dtype=torch.int32, device=dev)
            D.cosine_match_device(ctx, d_ref, d_cur, thr, idx)
            assert np.array_equal(idx.cpu().numpy(), want["force", thr]), (dim, thr)


@functools.lru_cache(maxsize=None)
def raster_case(n_cur):
    """64 reference rows against n_cur candidates of 64 components in raster order (bands of 4 rows of a 1024-wide image), window
    (30, 16), two NaN coordinates on each side; every row predicts a candidate planted for it to within 0.8 of the window."""
    n_ref, dim, col, row = 64, 64, 30, 16
    rs = np.random.RandomState(n_cur)
    ref = rs.standard_normal((n_ref, dim)).astype(np.float32)
    cur = rs.standard_normal((n_cur, dim)).astype(np.float32)
    cur_uv = np.stack([rs.uniform(0, 1024, n_cur), rs.uniform(0, 1024, n_cur)], axis=1).astype(np.float32)
    order = np.lexsort((cur_uv[:, 0], np.floor(cur_uv[:, 1] / 4)))
    cur_uv = cur_uv[order]
    partner = rs.choice(n_cur, size=n_ref, replace=False)
    cur[partner] = ref + np.float32(0.2) * rs.standard_normal((n_ref, dim)).astype(np.float32)
    pred_uv = (cur_uv[partner] + rs.uniform(-1, 1, size=(n_ref, 2)) * np.float32([col, row]) * 0.8).astype(np.float32)
    rorder = np.lexsort((pred_uv[:, 0], np.floor(pred_uv[:, 1] / 4)))
    ref, pred_uv = np.ascontiguousarray(ref[rorder]), np.ascontiguousarray(pred_uv[rorder])
    pred_uv[5] = np.nan
    pred_uv[n_ref // 2, 1] = np.nan
    cur_uv[7, 0] = np.nan
    cur_uv[n_cur - 3] = np.nan
    from tests import oracle_lib
    oracle_lib.lib()
    with np.errstate(all="ignore"):
        ok, want = oracle_lib.match_float(ref, cur, 0.45, pred_uv, cur_uv, max_col=col, max_row=row)
    assert ok and (want >= 0).sum() > n_ref // 2
    for a in (ref, cur, pred_uv, cur_uv, want):
        a.setflags(write=False)
    return ref, cur, pred_uv, cur_uv, want, (col, row)


@pytest.mark.parametrize("n_cur", [65600, 65536])
def test_more_cur_tiles_than_the_tile_list_holds(ftk, switch, n_cur):
    """NearbyMatch with 1 025 candidate tiles of 64, one more than the register-stationary kernel's tile list holds (kRrListCap): it must
    walk every tile without the list; and with exactly 1 024, the last size that has one."""
    switch("FTK_COSINE_SMALL", "0")
    ref, cur, pred_uv, cur_uv, want, (col, row) = raster_case(n_cur)
    with np.errstate(all="ignore"):
        ok, got = matcher(ftk, 0.45, col=col, row=row).NearbyMatch(ref, cur, pred_uv, cur_uv)
    assert ok is True
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:10], got[got != want][:10], want[got != want][:10])
