"""Every launch form of the device image pyramid (pyramid_kernels.hip through ftk_pyramid.cpp), byte for byte against the
numpy restatement in tests/pyramid_ref.py, at the tile, segment and vector edges.  No tolerances: a pyramid byte is right or wrong.

Which branch a shape reaches follows from ftk_layout: every level of a pyramid the library lays out starts on a 256-byte
boundary of one device block, and level l is (rows >> l) x (cols >> l) bytes with no row padding.

pyramid_fused_kernel<TW, TH> (levels 1..6; 256 x 16 tiles for a host / pinned source with <= 5 levels, 64 x 64 otherwise)
  * level-0 load, per 16-byte segment at column gc of a tile row: whole (gc + 16 <= cols), byte-wise tail (gc < cols < gc + 16),
    nothing (gc >= cols).  cols % 16 == 0 has no tail; cols < 16 has no whole segment; cols = 17, 65, 257, 273 ... have a tail of
    one byte, 15, 63, 255, 271 one of fifteen.  With `level0_keep` (a host / pinned source: the launch also writes the pyramid's
    own level 0) the keep store has the same three branches; without it (a device image, or after a copy) nothing is kept.
  * level store: level l's row gr starts at gr * (cols >> l) past a 256-aligned base and a thread's four pixels at a multiple of
    four columns, so the packed 32-bit store is taken when (gr * (cols >> l)) % 4 == 0 and all four pixels exist, the byte store
    otherwise: in the last partial group of a row, on three rows of four when the level width is odd (35, 17, 45, 11, ...), on
    every other row when it is 2 mod 4 (22), and always once a tile is narrower than four pixels (64 x 64 tiles, levels 5 and 6).

downsample_kernel (levels >= 7, from the level before; so only images at least 128 on both sides reach it)
  * `top` and `bottom` of a group are 8-byte aligned on every row iff the SOURCE level's width is a multiple of 8, and on no
    row otherwise (row 0's `bottom` is src + src_cols).  A level is therefore built by the vector branch alone or by the scalar
    loop alone: 512 -> level 6 is 8 wide -> level 7 vectorised; 576 -> 9 wide -> a full group of four, scalar; 1024 -> 16, 8 wide
    -> levels 7 and 8 vectorised; 1000 -> 15, 7 wide -> scalar groups of 4 + 3, then 3; 2049 -> 32, 16, 8 wide -> levels 7, 8, 9
    vectorised, then 4 and 2 wide -> levels 10 and 11 scalar (groups of 2 and 1).
  * UNREACHABLE for any pyramid the library lays out: the byte-wise `out` store inside the vector branch.  The branch needs a
    source width that is a multiple of 8, which makes the destination width a multiple of 4 and every `out` (256-aligned base +
    r * dst_cols + c0, c0 % 4 == 0) 4-byte aligned.  No shape is contrived for it.
"""
import ctypes as C

import numpy as np
import pytest

from tests import pyramid_cases as cases

pytestmark = pytest.mark.gpu

GUARD = 64       # sentinel bytes before and after a device source
SENTINEL = 0xA5


def assert_is_reference(pyr, kind, case, what):
    w, h, levels = case
    ref = cases.reference(kind, h, w, levels)
    assert pyr.level() == levels, (what, kind)
    for i in range(levels):
        got = pyr.download_level(i)
        assert got.shape == ref[i].shape, (what, kind, i, got.shape)
        if not np.array_equal(got, ref[i]):
            bad = np.argwhere(got != ref[i])
            r, c = bad[0]
            pytest.fail(f"{what}, {kind} {w} x {h} x {levels}: level {i} ({ref[i].shape[1]} x {ref[i].shape[0]}) differs in {len(bad)} of "
                        f"{ref[i].size} pixels, first at row {r} col {c}: {got[r, c]} where {ref[i][r, c]} is expected")


def other_image(kind, case):
    """A different image of the same shape, for the pyramid that is about to be refilled: the complement, so no byte of its
    level 0 equals the new image's.  On noise and coded its coarser levels differ from the new ones nearly everywhere as well,
    and those are what catch a stale level >= 1; on extremes they do not (the checkerboard half is 510 // 4 = 127 in both)."""
    w, h, _ = case
    return np.ascontiguousarray(255 - cases.image(kind, h, w))


class DeviceSource:
    """The image inside a larger flat device tensor: `offset` + 64 sentinel bytes, the image, 64 sentinel bytes.  The pointer is that
    of a slice of the flat tensor, so with offset 1 or 3 the image starts at an odd address."""

    def __init__(self, img, offset=0):
        import torch
        self.host = np.full(offset + GUARD + img.size + GUARD, SENTINEL, np.uint8)
        self.host[offset + GUARD: offset + GUARD + img.size] = img.ravel()
        self.tensor = torch.from_numpy(self.host.copy()).cuda()
        torch.cuda.synchronize()
        self.view = self.tensor[offset + GUARD: offset + GUARD + img.size]
        self.ptr = self.view.data_ptr()
        assert self.ptr == self.tensor.data_ptr() + offset + GUARD and self.tensor.data_ptr() % 256 == 0

    def assert_untouched(self, what):
        assert np.array_equal(self.tensor.cpu().numpy(), self.host), f"{what}: the source image or the bytes around it were written"


def pinned_source(img, offset=0):
    """(tensor to keep alive, pointer) of the image `offset` bytes into a pinned host allocation."""
    import torch
    flat = np.full(offset + img.size, SENTINEL, np.uint8)
    flat[offset:] = img.ravel()
    t = torch.from_numpy(flat).pin_memory()
    assert t.is_pinned()
    return t, t[offset:].data_ptr()


def build_device(ftk, kind, case, offset=0):
    """ImagePyramid.build_from_device: the square tile without keep; level 0 stays the caller's."""
    w, h, levels = case
    img = cases.image(kind, h, w)
    src = DeviceSource(img, offset)
    what = f"build_from_device(+{offset})"
    pyr = ftk.ImagePyramid.build_from_device(src.ptr, h, w, levels, keepalive=src.tensor)
    assert pyr.level_desc(0) == (src.ptr, h, w), what  # borrowed, not copied
    assert np.array_equal(pyr.download_level(0), img), (what, kind)
    assert_is_reference(pyr, kind, case, what)
    src.assert_untouched(what)
    pyr.close()


def update_device(ftk, kind, case, offset=0):
    """update(ptr, "device"): a device-to-device copy into level 0, then the square tile without keep."""
    w, h, levels = case
    src = DeviceSource(cases.image(kind, h, w), offset)
    pyr = ftk.ImagePyramid.build(other_image(kind, case), levels)
    pyr.update(src.ptr, "device")
    assert_is_reference(pyr, kind, case, f'update(+{offset}, "device")')
    src.assert_untouched("update from device memory")
    pyr.close()


def update_pinned(ftk, kind, case, offset=0):
    """update(ptr, "host_async") of pinned memory: the launch reads the frame itself and keeps level 0 (wide tile up to 5 levels,
    square tile at 6 and 7).  Memory the device cannot address takes the copy instead; the bytes must be the same either way."""
    w, h, levels = case
    keep, ptr = pinned_source(cases.image(kind, h, w), offset)
    assert ptr % 16 == offset
    pyr = ftk.ImagePyramid.build(other_image(kind, case), levels)
    pyr.update(ptr, "host_async")
    assert_is_reference(pyr, kind, case, f'update(pinned +{offset}, "host_async")')  # (download_level waits for the stream)
    assert np.array_equal(keep.numpy()[offset:], cases.image(kind, h, w).ravel()) and (keep.numpy()[:offset] == SENTINEL).all()
    pyr.close()


@pytest.mark.parametrize("case", cases.FORMS["build_host"], ids=cases.case_id)
def test_build_from_a_host_image(ftk, case):
    """ImagePyramid.build(host image, L): L = 1 a plain copy; L in 2..5 the wide tile with keep; L in 6..7 the square tile with
    keep; L >= 8 the square tile with keep, then downsample_kernel per level (branches per shape: module docstring)."""
    w, h, levels = case
    for kind in cases.KINDS:
        pyr = ftk.ImagePyramid.build(cases.image(kind, h, w), levels)
        assert_is_reference(pyr, kind, case, "build")
        pyr.close()


@pytest.mark.parametrize("case", cases.FORMS["build_device"], ids=cases.case_id)
def test_build_from_a_device_image(ftk, case):
    """ImagePyramid.build_from_device at every depth: the square tile WITHOUT keep (also at the wide-tile sizes, where a width
    below 16 has no whole segment), then downsample_kernel from level 7.  Level 0 is the caller's image, every level is
    downloaded, and neither the image nor the 64 bytes either side of it change."""
    for kind in cases.KINDS:
        build_device(ftk, kind, case)


@pytest.mark.parametrize("case", cases.FORMS["update_host"], ids=cases.case_id)
def test_update_from_a_host_image(ftk, case):
    """update(img): through a pinned slot, read by the launch, which keeps level 0 — wide tile up to 5 levels, square tile with
    keep at 6 and 7.  The pyramid held another image: every byte of every level must be the new one's."""
    w, h, levels = case
    for kind in cases.KINDS:
        pyr = ftk.ImagePyramid.build(other_image(kind, case), levels)
        pyr.update(cases.image(kind, h, w))
        assert_is_reference(pyr, kind, case, "update(host)")
        pyr.close()


@pytest.mark.parametrize("case", cases.FORMS["update_device"], ids=cases.case_id)
def test_update_from_a_device_image(ftk, case):
    for kind in cases.KINDS:
        update_device(ftk, kind, case)


@pytest.mark.parametrize("case", cases.FORMS["update_pinned"], ids=cases.case_id)
def test_update_from_a_pinned_frame(ftk, case):
    for kind in cases.KINDS:
        update_pinned(ftk, kind, case)


@pytest.mark.parametrize("case", cases.FORMS["update_pageable"], ids=cases.case_id)
def test_update_from_a_pageable_frame_given_as_host_async(ftk, case):
    """update(ptr, "host_async") of memory that is not pinned: the copy path, then the square tile without keep."""
    w, h, levels = case
    for kind in cases.KINDS:
        frame = np.array(cases.image(kind, h, w))  # a private, pageable copy
        pyr = ftk.ImagePyramid.build(other_image(kind, case), levels)
        pyr.update(int(frame.ctypes.data), "host_async")
        assert_is_reference(pyr, kind, case, 'update(pageable, "host_async")')
        assert np.array_equal(frame, cases.image(kind, h, w))
        pyr.close()


@pytest.mark.parametrize("case", cases.FORMS["misaligned"], ids=cases.case_id)
@pytest.mark.parametrize("offset", cases.MISALIGNED_OFFSETS)
@pytest.mark.parametrize("form", [build_device, update_device, update_pinned], ids=lambda f: f.__name__)
def test_sources_at_odd_addresses(ftk, form, offset, case):
    """The device image and the pinned frame start 1 and 3 bytes into their allocation (the pointer of t[1:] / t[3:] of a flat
    tensor): every 16-byte segment load of the fused kernel is unaligned, and so is the level-0 download of a borrowed image."""
    for kind in cases.KINDS:
        form(ftk, kind, case, offset)


def test_refused_builds_leave_nothing_behind_and_the_context_usable(ftk):
    """A level that would be empty (8 x 8 x 5: 8, 4, 2, 1, 0), more than FTK_MAX_LEVELS levels (13, on an image that would hold
    them) and no level at all are refused from host and from device memory: the call raises, the C entry hands no pyramid
    back, and the same context then builds a correct pyramid."""
    import torch
    from feature_tracker_amd import _native as N
    ctx = ftk.default_context()
    for (w, h, levels) in [(8, 8, 5), (9, 300, 5), (8, 8, 13), (4096, 4096, 13), (8, 8, 0)]:
        img = np.zeros((h, w), np.uint8)
        d_img = torch.from_numpy(img).cuda()
        torch.cuda.synchronize()
        with pytest.raises(N.FtkError):
            ftk.ImagePyramid.build(img, levels)
        with pytest.raises(N.FtkError):
            ftk.ImagePyramid.build_from_device(d_img.data_ptr(), h, w, levels, keepalive=d_img)
        for on_device, ptr in ((0, img.ctypes.data), (1, d_img.data_ptr())):
            out = C.c_void_p()
            rc = N.lib().ftk_pyramid_build(ctx.handle, C.c_void_p(ptr), h, w, levels, on_device, C.byref(out))
            assert rc != 0 and not out, (w, h, levels, on_device)
    for case in [(16, 16, 5), (64, 64, 7)]:
        w, h, levels = case
        for kind in cases.KINDS:
            pyr = ftk.ImagePyramid.build(cases.image(kind, h, w), levels)
            assert_is_reference(pyr, kind, case, "build after a refusal")
            pyr.close()
            build_device(ftk, kind, case)


# (u, v) for the extended-patch extractor on a 40 x 30 image: non-finite, beyond int32, the largest float below 2^31 and -2^31
# itself (the ends of the range the float -> int conversion accepts), -0.0, and exactly on / one past the last valid lattice
# column (cols - 2) and row (rows - 2)
PATCH_IMAGE = (30, 40)  # rows, cols
NAN, INF = float("nan"), float("inf")
PATCH_POSITIONS = [(20.3, 15.7), (NAN, 15.5), (20.5, NAN), (NAN, NAN), (INF, 15.5), (-INF, 15.5), (20.5, INF), (20.5, -INF), (INF, -INF),
                   (1e30, 15.5), (-1e30, 15.5), (20.5, 1e30), (20.5, -1e30), (2147483520.0, 15.5), (20.5, 2147483520.0), (2147483520.0, 2147483520.0),
                   (-2147483648.0, 15.5), (20.5, -2147483648.0), (2147483648.0, 15.5), (-0.0, -0.0), (-0.0, 15.5), (20.25, -0.0), (0.0, 0.0),
                   (38.0, 28.0), (38.0, 10.25), (20.75, 28.0), (38.5, 28.5), (39.0, 29.0), (37.999996, 27.999998)]
# rows x cols: the existing odd patch, an even one of exactly 64 elements (one pass of the 64-lane loop), 65 elements (a second pass
# for one lane), 64 in one row, a single pixel, and a patch larger than the image
PATCH_SHAPES = [(9, 11), (8, 8), (5, 13), (1, 64), (1, 1), (35, 45)]


@pytest.mark.parametrize("shape", PATCH_SHAPES, ids=lambda s: "%dx%d" % s)
def test_extract_extend_patch_at_the_edges_of_its_arguments(ftk, oracle, shape):
    """ExtractExtendPatchInReferenceImage == the oracle's in count, validity and patch bits, at positions that are non-finite, wrap
    the integer lattice or sit exactly on the last valid column / row, for patch sizes around the 64-lane loop's edge."""
    img = np.array(cases.image("noise", *PATCH_IMAGE))
    pyr = ftk.ImagePyramid.from_host_levels([img])
    klt = ftk.OpticalFlowBasicKlt()
    some_valid = 0
    for (u, v) in PATCH_POSITIONS:
        cnt, patch, valid = klt.ExtractExtendPatchInReferenceImage(pyr, (u, v), *shape)
        ocnt, opatch, ovalid = oracle.extract_extend_patch(img, u, v, *shape)
        assert cnt == ocnt == int(valid.sum()), (u, v)
        assert np.array_equal(valid, ovalid.astype(bool)), (u, v)
        assert np.array_equal(patch.view(np.uint32), opatch.view(np.uint32)), (u, v)
        assert not patch[~valid].view(np.uint32).any(), (u, v)  # +0.0 wherever the lattice leaves the image
        if not (np.isfinite(u) and np.isfinite(v) and abs(u) < 1e6 and abs(v) < 1e6):
            assert cnt == 0, (u, v)
        some_valid += cnt
    assert some_valid > 0
    if shape == (35, 45):  # larger than the image: at its centre every lattice pixel of the image is there, and no more
        cnt, _, valid = klt.ExtractExtendPatchInReferenceImage(pyr, (20.3, 15.7), *shape)
        assert cnt == (PATCH_IMAGE[0] - 1) * (PATCH_IMAGE[1] - 1)


@pytest.mark.parametrize("kind", cases.HARRIS_KINDS)
@pytest.mark.parametrize("size", cases.HARRIS_SIZES, ids=lambda s: "%dx%d" % s)
def test_harris_on_saturated_and_noisy_content(ftk, oracle, kind, size):
    """Harris response (bit-exact) and detection against the oracle on content the smooth test images never have.  What each
    image delivers is asserted by tests/test_pyramid_ref_cpu.py::test_harris_images_reach_the_range_they_are_there_for:
      extremes: one seam of |gx| = 510 beside a checkerboard without any gradient; two responses besides 0, so the suppression
                has to order exactly equal candidates by pixel index
      noise:    |g| up to about 870, sums up to about 5.5e6 — every sum still exact in fp32
      stripes:  |gx| = 1020 (upper half) and |gy| = 1020 (lower half), the ends of the Sobel range, on every pixel; 5 x 5 sums of
                25 * 1020^2 = 26 010 000 > 2^24; equal responses over whole regions
      jitter:   stripes with noise in the two low bits: sums beyond 2^24 built from odd products, where an fp32 accumulation
                rounds (45 % of the windows) and the response bits change — the image a narrowed or float sum fails on."""
    w, h = size
    img = np.array(cases.image(kind, h, w))
    det = ftk.FeaturePointHarrisDetector()
    got = det.response(img)
    exp = oracle.harris_response(img)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert np.abs(exp).max() > 0
    for dist in (1, 5):
        for max_n, thr in ((100000, 40.0), (50, 40.0), (100000, -1e30)):
            det.options().kMinFeatureDistance, det.options().kMinValidResponse = dist, thr
            ok, uv = det.DetectGoodFeatures(img, max_n)
            want = oracle.harris_detect(img, max_n, dist, thr)
            assert ok and uv.shape == want.shape and np.array_equal(uv, want), (dist, max_n, thr)
        assert len(want) > 0  # (at a threshold of -1e30 every centre is a candidate)
