"""GPU parity tests: the Hamming matcher at EVERY descriptor width, against tests/hamming_ref.py (the numpy restatement of
descriptor_matcher.h) and against the C oracle, so that a disagreement names which of the three is the odd one.  Indices are compared
exactly everywhere.

ftk_hamming_match / ftk_hamming_match_device pick one of five scan forms from the width (csrc/match_plan.cpp): Small (one launch, any
padded width up to 16 words), Popcount (1, 2, 4, 8, 16 words), MatrixCores (8, 16 words), Plain (n_bits == 0) and Generic (more than
16 words); widths 3, 5..7 and 9..15 words are zero-padded to the next instantiated width, by the host entry during its gather and by
the device entry in pad_descriptors.  tests/test_matcher_gpu.py runs 64, 128, 200, 256 and 512 bits; here:

  * the width-and-shape sweep of hamming_ref.sweep_params() through the host entry, under the default dispatch and FTK_MATCH_SMALL=0,
    and FTK_MATCH_KERNEL unset / mfma / scalar where the width has both scans;
  * the Generic form with prediction windows and >= 2048 candidates (boxes reserved, not launched);
  * the device entry with 3, 7, 9, 15 and 17 words: pad_descriptors, its buffer regrown and reused, a caller's workspace;
  * brief_compute_device -> hamming_match_device at 32 bits (one word);
  * the matrix-core scan with 1024 whole tiles in one split, the size of its keys' position field.

hamming_calls() lists every (n_bits, shape, switches) run here; tests/test_hamming_ref_cpu.py walks their plans on the CPU and holds
that every form, instantiated width and pad is among them."""
import functools

import numpy as np
import pytest

from tests import hamming_ref as H

pytestmark = pytest.mark.gpu

COL, ROW = H.SWEEP_WINDOW
SWEEP = H.sweep_params()
KERNELS = (None, "mfma", "scalar")                   # FTK_MATCH_KERNEL
GENERIC_WINDOWS = (544, 200, 2100)                   # (n_bits, n_ref, n_cur): >= 2048 candidates
DEVICE_BITS = (96, 200, 257, 480, 544)               # 3, 7, 9, 15, 17 words
DEVICE_SHAPES = ((65, 33), (130, 95), (40, 24))      # then a larger, then a smaller call on the same context
BRIEF_MATCH = (32, 300, 280)
SPLIT_CAP = (256, 65537, 32768 + 64)
PLAIN = (0, 65, 33)


def both_scans(n_bits):
    return 5 <= (n_bits + 31) // 32 <= 16  # 8 or 16 words on the device: matrix cores and popcount


def hamming_calls():
    """((n_bits, n_ref, n_cur), FTK_MATCH_SMALL, FTK_MATCH_KERNEL as the plan reads it, nearby) of every matcher call of this module."""
    calls = []
    for small in (None, 0):
        for case in SWEEP + [GENERIC_WINDOWS, PLAIN] + [(b, r, c) for b in DEVICE_BITS for r, c in DEVICE_SHAPES] + [BRIEF_MATCH]:
            for kernel in ((None, 1, 0) if both_scans(case[0]) and case in SWEEP else (None,)):
                calls += [(case, small, kernel, nearby) for nearby in (0, 1)]
    return calls + [(SPLIT_CAP, 0, None, nearby) for nearby in (0, 1)]


@pytest.fixture(params=["default", "launches"])
def matcher_form(request, switch):
    """As in tests/test_matcher_gpu.py: the default dispatch, and the one-launch form switched off (FTK_MATCH_SMALL=0, read per call), so
    that small inputs also reach the kernels that serve the large ones."""
    if request.param == "launches":
        switch("FTK_MATCH_SMALL", "0")
    return request.param


def matcher(ftk, max_dist, col=COL, row=ROW):
    m = ftk.BriefMatcher()
    m.options().kMaxValidDescriptorDistance = max_dist
    m.options().kMaxValidPredictColDistance = col
    m.options().kMaxValidPredictRowDistance = row
    return m


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def same(got, want_ref, want_oracle, what):
    """Exact equality of the three; the message says who stands alone."""
    if np.array_equal(got, want_ref) and np.array_equal(got, want_oracle):
        return
    if np.array_equal(want_ref, want_oracle):
        odd = "the kernel differs from hamming_ref and the oracle, which agree"
    elif np.array_equal(got, want_oracle):
        odd = "hamming_ref differs from the kernel and the oracle, which agree"
    elif np.array_equal(got, want_ref):
        odd = "the oracle differs from the kernel and hamming_ref, which agree"
    else:
        odd = "all three differ"
    rows = np.flatnonzero((got != want_ref) | (got != want_oracle))[:8]
    raise AssertionError(f"{what}: {odd}; rows {rows.tolist()}: kernel {got[rows].tolist()}, hamming_ref {want_ref[rows].tolist()}, oracle {want_oracle[rows].tolist()}")


def expectations(c, windows, thresholds):
    """{(thr, window or None): (hamming_ref, oracle)} of a case, computed once."""
    from tests import oracle_lib
    oracle_lib.lib()
    D = H.distances(c.ref, c.cur)
    want = {}
    with np.errstate(invalid="ignore"):
        for thr in thresholds:
            want[thr, None] = (H.force_match(c.ref, c.cur, thr, c.stale, D=D)[1], oracle_lib.force_match(c.ref, c.cur, thr, c.stale)[1])
            for col, row in windows:
                want[thr, (col, row)] = (H.nearby_match(c.ref, c.cur, c.pred_uv, c.cur_uv, thr, col, row, c.stale, D=D)[1],
                                         oracle_lib.nearby_match(c.ref, c.cur, c.pred_uv, c.cur_uv, thr, col, row, c.stale)[1])
    for pair in want.values():
        frozen(*pair)
    return D, want


@functools.lru_cache(maxsize=None)
def sweep_reference(n_bits, n_ref, n_cur):
    c = H.sweep_case(n_bits, n_ref, n_cur)
    frozen(c.ref, c.cur, c.pred_uv, c.cur_uv, c.stale)
    D, want = expectations(c, [(COL, ROW)], c.thresholds)
    H.assert_case_is_telling(c, D)
    return c, want


def run_host(ftk, c, want, what):
    for (thr, window), (want_ref, want_oracle) in want.items():
        with np.errstate(invalid="ignore"):
            if window is None:
                ok, got = matcher(ftk, thr).ForceMatch(c.ref, c.cur, c.stale.copy())
            else:
                ok, got = matcher(ftk, thr, *window).NearbyMatch(c.ref, c.cur, c.pred_uv, c.cur_uv, c.stale.copy())
        assert ok is True
        same(got, want_ref, want_oracle, what + (thr, window))


@pytest.mark.parametrize("n_bits,n_ref,n_cur", SWEEP)
def test_width_sweep_host_entry(ftk, switch, matcher_form, n_bits, n_ref, n_cur):
    """Every width of the sweep at the ragged ends of the 64-row, 512-row and 32-candidate tiles: thresholds 0, the planted distance (at
    which no planted pair may match), just above it, 60 and 3e9; a duplicate candidate, all-zero rows, NaN coordinates, a candidate on
    the window's edge and stale indices (hamming_ref.sweep_case)."""
    c, want = sweep_reference(n_bits, n_ref, n_cur)
    assert set(t for t, _ in want) == {0.0, float(c.flips), c.flips + 0.5, 60.0, 3e9} and c.flips == max(1, n_bits // 12)
    for kernel in KERNELS if both_scans(n_bits) else (None,):
        switch("FTK_MATCH_KERNEL", kernel)
        run_host(ftk, c, want, (matcher_form, kernel, n_bits, n_ref, n_cur))


def test_no_bits_plain_scan(ftk, matcher_form):
    """n_bits == 0, the Plain form: ComputeDistance is kMaxInt32 for every pair, so candidate 0 under a threshold above 2^31 and nothing below."""
    n_bits, n_ref, n_cur = PLAIN
    c = H.sweep_case(8, n_ref, n_cur)
    c.ref, c.cur = c.ref[:, :0], c.cur[:, :0]
    _, want = expectations(c, [(COL, ROW)], (60.0, 2147483648.0, 3e9))
    assert (want[3e9, None][0] == 0).all() and np.array_equal(want[60.0, None][0], c.stale)
    run_host(ftk, c, want, (matcher_form, n_bits, n_ref, n_cur))


@functools.lru_cache(maxsize=None)
def generic_reference():
    """544 bits in raster order (both lists sorted by 4-pixel bands, then by u), so that most row blocks and candidate splits are out
    of each other's reach: the Popcount and MatrixCores scans leave early on their boxes there; Generic has no such exit and must
    not need one.  Half of the partnered rows are predicted exactly ON their candidate (the window of zero keeps only those)."""
    n_bits, n_ref, n_cur = GENERIC_WINDOWS
    rs = np.random.RandomState(544)
    flips = n_bits // 12
    ref, cur, partner = H.planted(rs, n_bits, n_ref, n_cur, flips)
    cur_uv = rs.uniform(0, 752, size=(n_cur, 2)).astype(np.float32)
    pred_uv = rs.uniform(0, 752, size=(n_ref, 2)).astype(np.float32)
    rows, first = np.unique(partner[partner >= 0], return_index=True)  # each partnered row and the first candidate planted from it
    first = np.flatnonzero(partner >= 0)[first]
    how = rs.random_sample(rows.size)
    on, off = how < 0.5, (how >= 0.5) & (how < 0.75)  # exactly on the candidate | within the (35, 80) window of it | anywhere
    pred_uv[rows[on]] = cur_uv[first[on]]
    pred_uv[rows[off]] = cur_uv[first[off]] + rs.uniform(-28, 28, size=(int(off.sum()), 2)).astype(np.float32)
    c_order = np.lexsort((cur_uv[:, 0], np.floor(cur_uv[:, 1] / 4)))
    r_order = np.lexsort((pred_uv[:, 0], np.floor(pred_uv[:, 1] / 4)))
    ref, pred_uv = np.ascontiguousarray(ref[r_order]), np.ascontiguousarray(pred_uv[r_order])
    cur, cur_uv = np.ascontiguousarray(cur[c_order]), np.ascontiguousarray(cur_uv[c_order])
    cur[n_cur - 5] = cur[40]  # a duplicate 2000 candidates further down
    cur_uv[n_cur - 5] = cur_uv[40]
    pred_uv[5] = np.nan
    pred_uv[n_ref // 2, 1] = np.nan
    cur_uv[7, 0] = np.nan
    cur_uv[n_cur - 3] = np.nan
    c = H.Case(n_bits, flips, ref, cur, pred_uv, cur_uv, np.arange(n_ref, dtype=np.int32) + 7000, partner, (0.0, float(flips), flips + 0.5, 60.0, 3e9))
    frozen(c.ref, c.cur, c.pred_uv, c.cur_uv, c.stale)
    D, want = expectations(c, [(COL, ROW), (0, 0)], c.thresholds)
    for window in ((COL, ROW), (0, 0)):
        got = want[60.0, window][0]
        assert (got < 7000).sum() > 20 and (got >= 7000).sum() > 20, window  # some rows match, some do not
    return c, want


def test_generic_form_with_windows_and_many_candidates(ftk, matcher_form):
    """The Generic kernel (17 words) under NearbyMatch with n_cur >= 2048, where the plan reserves boxes that this form never launches."""
    c, want = generic_reference()
    run_host(ftk, c, want, (matcher_form,) + GENERIC_WINDOWS)


@pytest.mark.parametrize("n_bits", DEVICE_BITS)
def test_device_entry_pads_on_the_device(ftk, matcher_form, n_bits):
    """hamming_match_device on tensors of 3, 7, 9, 15 and 17 words: the first four are padded on the device (pad_descriptors, two
    strided copies into the context's match_pad), 17 words go to the Generic kernel as they are.  ForceMatch and NearbyMatch, with
    the context's keys and with a caller's workspace; then a larger and a smaller call on the SAME context, so that match_pad is regrown
    and then reused with room to spare (what lies beyond the smaller call's rows must not count).  The caller's tensors are not written."""
    import torch
    from feature_tracker_amd import device as D
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        ctx = D.context_on_stream(stream, 0)
        for n_ref, n_cur in DEVICE_SHAPES:
            c, want = sweep_reference(n_bits, n_ref, n_cur)
            words_ref, words_cur = ftk.pack_brief(c.ref), ftk.pack_brief(c.cur)
            assert words_ref.shape[1] == (n_bits + 31) // 32
            given = [torch.from_numpy(a.view(np.int32).copy()).to(dev) for a in (words_ref, words_cur, c.pred_uv, c.cur_uv)]
            d_ref, d_cur, d_pred, d_cuv = given
            d_pred, d_cuv = d_pred.view(torch.float32), d_cuv.view(torch.float32)
            kept = [t.clone() for t in given]
            for (thr, window), (want_ref, want_oracle) in want.items():
                for workspace in (None, torch.full((n_ref + 3,), 5, dtype=torch.int64, device=dev)):
                    d_idx = torch.from_numpy(c.stale.copy()).to(dev)
                    if window is None:
                        D.hamming_match_device(ctx, d_ref, d_cur, n_bits, thr, d_idx, workspace=workspace)
                    else:
                        D.hamming_match_device(ctx, d_ref, d_cur, n_bits, thr, d_idx, pred_uv=d_pred, cur_uv=d_cuv, max_col=window[0], max_row=window[1],
                                               workspace=workspace)
                    stream.synchronize()
                    same(d_idx.cpu().numpy(), want_ref, want_oracle, (matcher_form, n_bits, n_ref, n_cur, thr, window, workspace is not None))
            for t, k in zip(given, kept):
                assert torch.equal(t, k)  # (compared as int32: NaN coordinates included)


@pytest.mark.parametrize("half", [1, 8])
def test_brief_to_match_at_32_bits_on_device(ftk, oracle, matcher_form, half):
    """brief_compute_device(32 bits) -> hamming_match_device with no host hop: one-word descriptors, which BriefDescriptor produces and
    nothing matched.  Distances are 0..32, so ties are the rule: the lowest index must win throughout."""
    import torch
    from feature_tracker_amd import device as D
    from feature_tracker_amd import synth
    n_bits, n_ref, n_cur = BRIEF_MATCH
    ref_img, cur_img = synth.make_image_pair(320, 240, (3.3, -2.1))
    rs = np.random.RandomState(32 + half)
    ref_uv = np.stack([rs.uniform(-5, 325, n_ref), rs.uniform(-5, 245, n_ref)], axis=1).astype(np.float32)
    cur_uv = (ref_uv[rs.permutation(n_ref)[:n_cur]] + np.float32([3.3, -2.1])).astype(np.float32)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    _, rb = oracle.brief_compute(ref_img, ref_uv, n_bits, half)
    _, cb = oracle.brief_compute(cur_img, cur_uv, n_bits, half)
    assert rb.any(axis=1).sum() > n_ref // 2 and not rb.all(axis=1).any()
    with torch.cuda.stream(stream):
        ctx = D.context_on_stream(stream, 0)
        rp, cp = D.upload_pyramid([ref_img], ctx, dev), D.upload_pyramid([cur_img], ctx, dev)
        d_ruv, d_cuv = torch.from_numpy(ref_uv).to(dev), torch.from_numpy(cur_uv).to(dev)
        d_rw = torch.zeros((n_ref, 1), dtype=torch.int32, device=dev)
        d_cw = torch.zeros((n_cur, 1), dtype=torch.int32, device=dev)
        D.brief_compute_device(ctx, rp, d_ruv, n_bits, half, d_rw)
        D.brief_compute_device(ctx, cp, d_cuv, n_bits, half, d_cw)
        seen = False
        for thr in (0.0, 1.0, 3.0, 6.5, 3e9):
            for window in (None, (50, 50)):
                d_idx = torch.full((n_ref,), -1, dtype=torch.int32, device=dev)
                if window is None:
                    D.hamming_match_device(ctx, d_rw, d_cw, n_bits, thr, d_idx)
                    want_ref, want_oracle = H.force_match(rb, cb, thr)[1], oracle.force_match(rb, cb, thr)[1]
                else:
                    D.hamming_match_device(ctx, d_rw, d_cw, n_bits, thr, d_idx, pred_uv=d_ruv, cur_uv=d_cuv, max_col=window[0], max_row=window[1])
                    want_ref = H.nearby_match(rb, cb, ref_uv, cur_uv, thr, window[0], window[1])[1]
                    want_oracle = oracle.nearby_match(rb, cb, ref_uv, cur_uv, thr, window[0], window[1])[1]
                stream.synchronize()
                same(d_idx.cpu().numpy(), want_ref, want_oracle, (matcher_form, half, thr, window))
                seen |= bool((want_ref >= 0).any() and (want_ref < 0).any())
        assert seen
        assert np.array_equal(d_rw.cpu().numpy().view(np.uint32), ftk.pack_brief(rb))


# ---- the matrix-core scan's split cap ----

TILE = 32
CAP_TILES = 1024  # kMfmaMaxTilesPerSplit: the position field of the running keys


@functools.lru_cache(maxsize=None)
def split_cap_inputs():
    """256 bits, 65 537 rows (1025 waves, so one wave walks all candidates of a split), 32 832 candidates = 1026 tiles: a split of 1024
    whole tiles and a second of two.  Random descriptors (unrelated pairs sit near 128 +- 8 bits: none of the 2 x 10^9 comes near 60);
    reference row k of `rows` has its partner (20 flips) at candidate `at[k]`: in tiles 0, 1022, 1023, 1024 and the last one (whole at
    this size: 32 832 = 1026 x 32), at the first and last lanes of the tiles beside the cap.  Two rows have exact duplicates of their
    partner on both sides of the 1023 | 1024 boundary: the lower index must win, within a split and across the two."""
    n_bits, n_ref, n_cur = SPLIT_CAP
    rs = np.random.RandomState(1024)
    ref = rs.randint(0, 2, size=(n_ref, n_bits)).astype(np.uint8)
    cur = rs.randint(0, 2, size=(n_cur, n_bits)).astype(np.uint8)
    at = np.array([0, 31, 1022 * TILE, 1022 * TILE + 31, 1023 * TILE, 1023 * TILE + 30, 1023 * TILE + 31, 1024 * TILE + 1, 1024 * TILE + 2, 1024 * TILE + 31,
                   1025 * TILE, n_cur - 1])
    rows = np.array([0, 63, 64, 4097, 65535, 65536, 32768, 1, 33000, 12345, 65500, 40000])
    for i, j in zip(rows, at):
        cur[j] = ref[i]
        cur[j, rs.permutation(n_bits)[:20]] ^= 1
    # duplicates: row 4097's partner (tile 1022) again in tiles 1023 and 1024; row 32768's (the last lane of tile 1023) again at the first lane of tile 1024
    cur[1023 * TILE + 7] = cur[at[3]]
    cur[1024 * TILE + 9] = cur[at[3]]
    cur[1024 * TILE] = cur[at[6]]
    want = dict(zip(rows.tolist(), at.tolist()))
    extra = np.setdiff1d(rs.permutation(n_ref)[:400], rows)[: 256 - rows.size]
    sample = np.sort(np.concatenate([rows, extra]))
    assert sample.size == 256 and np.isin(rows, sample).all()
    uv_ref, uv_cur = np.full((n_ref, 2), 100.0, np.float32), np.full((n_cur, 2), 100.0, np.float32)
    ok, sampled = H.force_match(ref[sample], cur, 60.0)
    assert ok and all(sampled[np.searchsorted(sample, i)] == j for i, j in want.items())
    assert (sampled >= 0).sum() == len(want)
    frozen(ref, cur, sample, sampled, uv_ref, uv_cur)
    return ref, cur, sample, sampled, uv_ref, uv_cur


def test_split_cap_plan():
    """The shape still gives what the test below is there for: one wave per 64 rows, a split of 1024 tiles and a short second one."""
    from tests.test_match_plan_cpu import plan
    n_bits, n_ref, n_cur = SPLIT_CAP
    for nearby in (0, 1):
        p, = plan("hamming", [dict(n_ref=n_ref, n_cur=n_cur, n_words=8, n_bits=n_bits, nearby=nearby, small=0)])
        assert p["form"] == "matrix_cores" and p["dev_words"] == 8 and p["pad"] == 0
        assert p["cur_per_block"] == CAP_TILES * TILE and p["scan_grid"] == (1025, 2) and p["scan_block"] == (64, 1)
        assert (p["box_grid"][0] > 0) == bool(nearby)


@pytest.mark.parametrize("nearby", [False, True])
def test_split_of_1024_whole_tiles(ftk, switch, nearby):
    """A position that wrapped, or keys that ordered wrongly, at tile 1023 -> 1024 would send a planted row to another candidate.  A full
    brute force on the CPU is out of reach (2 x 10^9 pairs), so: (a) hamming_ref on 256 rows — every planted row, every duplicate's
    row, 244 others — against all candidates, exactly; (b) for ALL rows, the index is -1 or in range and the distance of that one
    pair, recounted here, is below the threshold; rows outside the sample that matched must be none (see split_cap_inputs)."""
    switch("FTK_MATCH_SMALL", "0")
    ref, cur, sample, sampled, uv_ref, uv_cur = split_cap_inputs()
    n_ref, n_cur = ref.shape[0], cur.shape[0]
    thr = 60.0
    m = matcher(ftk, thr, 40, 40)
    ok, got = m.NearbyMatch(ref, cur, uv_ref, uv_cur) if nearby else m.ForceMatch(ref, cur)  # all coordinates equal: every window passes
    assert ok is True and got.shape == (n_ref,) and got.dtype == np.int32
    assert np.array_equal(got[sample], sampled), (sample[got[sample] != sampled], got[sample][got[sample] != sampled], sampled[got[sample] != sampled])
    assert ((got >= -1) & (got < n_cur)).all()
    hit = np.flatnonzero(got >= 0)
    recount = (ref[hit] != cur[got[hit]]).sum(axis=1)
    assert (recount.astype(np.float32) < np.float32(thr)).all()
    assert np.isin(hit, sample).all()
