"""CPU companion of tests/test_pyramid_gpu.py: the two references the device pyramids are held to — the oracle's C
CreateImagePyramid and the numpy restatement in tests/pyramid_ref.py — are pinned to each other on every (image kind, size,
levels) tuple the GPU file uses, before anything runs on a GPU; and the images are shown to tell a wrong pyramid from a right one."""
import numpy as np
import pytest

from tests import pyramid_cases as cases
from tests import pyramid_ref


@pytest.mark.parametrize("case", cases.all_cases(), ids=cases.case_id)
def test_oracle_pyramid_equals_the_restatement(oracle, case):
    w, h, levels = case
    for kind in cases.KINDS:
        img = cases.image(kind, h, w)
        ref = cases.reference(kind, h, w, levels)
        got = oracle.create_pyramid(img.copy(), levels)
        assert len(got) == len(ref) == levels
        for i in range(levels):
            assert got[i].shape == ref[i].shape == (h >> i, w >> i), (kind, i)
            assert np.array_equal(got[i], ref[i]), (kind, i)


def test_the_restatement_on_a_pyramid_worked_by_hand():
    img = np.uint8([[1, 2, 9, 9, 7],
                    [3, 5, 9, 8, 7],
                    [255, 255, 0, 0, 7],
                    [255, 254, 1, 2, 7],
                    [6, 6, 6, 6, 6]])
    l0, l1, l2 = pyramid_ref.pyramid(img, 3)
    assert np.array_equal(l0, img)
    assert np.array_equal(l1, np.uint8([[2, 8], [254, 0]]))  # 11 // 4, 35 // 4, 1019 // 4, 3 // 4; row 4 and column 4 dropped
    assert np.array_equal(l2, np.uint8([[66]]))              # (2 + 8 + 254 + 0) // 4: the mean of level 1's BYTES
    assert pyramid_ref.max_levels(5, 5) == 3 and pyramid_ref.max_levels(8, 8) == 4 and pyramid_ref.max_levels(2050, 2049) == 12
    for too_many in (0, 4):
        with pytest.raises(ValueError):
            pyramid_ref.pyramid(img, too_many)


def test_image_kinds_are_pure_functions_with_the_promised_content():
    for kind in cases.KINDS:
        a = cases.image(kind, 33, 70)
        b = cases.image.__wrapped__(kind, 33, 70)  # computed afresh, not from the cache
        assert a.dtype == np.uint8 and a.shape == (33, 70) and np.array_equal(a, b)
        assert not a.flags.writeable  # shared between tests: nobody changes it
    coded = cases.image("coded", 64, 300).astype(np.int32)
    assert (coded[:, 1:] != coded[:, :-1]).all() and (coded[1:] != coded[:-1]).all()
    assert (coded[1:, 1:] != coded[:-1, :-1]).all() and (coded[1:, :-1] != coded[:-1, 1:]).all()
    ext = cases.image("extremes", 16, 64).astype(np.int32)
    assert set(np.unique(ext)) == {0, 255}
    sums = ext[0::2, 0::2] + ext[0::2, 1::2] + ext[1::2, 0::2] + ext[1::2, 1::2]
    assert set(np.unique(sums)) == {510, 1020}
    noise = cases.image("noise", 128, 512)
    assert len(np.unique(noise)) == 256 and not np.array_equal(noise, cases.image("noise", 128, 513)[:, :512])


@pytest.mark.parametrize("rows,cols", [(64, 64), (128, 512)])
def test_noise_tells_the_plausible_wrong_pyramids_from_the_right_one(rows, cols):
    """Two pyramids a kernel could produce by mistake must differ from the restatement in at least 10 % of the pixels of a noise
    image: level 2 as the floor mean of its 16 SOURCE pixels (instead of level 1's bytes), and level 1 rounded to nearest.
    (Measured: 28.5 % and 51.2 % at 64 x 64, 27.9 % and 50.6 % at 128 x 512.)"""
    img = cases.image("noise", rows, cols)
    ref = cases.reference("noise", rows, cols, 3)
    p = img.astype(np.uint32)
    r2, c2 = rows // 4, cols // 4
    of_source = (p[: 4 * r2, : 4 * c2].reshape(r2, 4, c2, 4).sum(axis=(1, 3)) // 16).astype(np.uint8)
    share = np.mean(of_source != ref[2])
    print(f"{rows} x {cols}: level 2 as the mean of 16 source pixels differs in {100 * share:.1f} %")
    assert share >= 0.10
    quads = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    rounded = ((quads + 2) // 4).astype(np.uint8)
    share = np.mean(rounded != ref[1])
    print(f"{rows} x {cols}: level 1 rounded to nearest differs in {100 * share:.1f} %")
    assert share >= 0.10


def test_case_tables_hold_the_sizes_they_are_there_for():
    """The properties that make the tables worth running: every tile-edge width and height more than once, five levels wherever a
    wide-tile size allows them, the odd level widths, the per-level shapes, and nothing deeper than its size allows."""
    for table in (cases.WIDE, cases.WIDE_TRIMMED):
        for w in cases.WIDE_WIDTHS:
            assert sum(1 for c in table if c[0] == w) >= 2, w
            if w >= 16:
                assert any(c[0] == w and c[1] >= 16 and c[2] == 5 for c in table), w
        for h in cases.WIDE_HEIGHTS:
            assert sum(1 for c in table if c[1] == h) >= 2, h
            if h >= 16:
                assert any(c[1] == h and c[0] >= 16 and c[2] == 5 for c in table), h
        assert (16, 16, 5) in table and (2, 2, 2) in table
        assert all(n <= 5 for _, _, n in table)
    for w in cases.SQUARE_WIDTHS:
        assert sum(1 for c in cases.SQUARE if c[0] == w) >= 2, w
    for h in cases.SQUARE_HEIGHTS:
        assert sum(1 for c in cases.SQUARE if c[1] == h) >= 2, h
    assert {n for _, _, n in cases.SQUARE} == {2, 6, 7}
    assert (128, 128, 7) in cases.SQUARE and (64, 64, 7) in cases.SQUARE
    assert [70 >> i for i in range(3)] == [70, 35, 17] and [90 >> i for i in range(3)] == [90, 45, 22]
    assert any(c[0] == 70 and c[2] >= 4 for c in cases.SQUARE) and any(c[0] == 90 and c[2] >= 4 for c in cases.SQUARE)
    assert cases.DEEP == [(512, 128, 8), (576, 130, 8), (1024, 256, 9), (1000, 300, 9), (2049, 2050, 12)]
    assert max(n for _, _, n in cases.all_cases()) == cases.MAX_LEVELS
    for w, h, n in cases.all_cases():
        assert 1 <= n <= pyramid_ref.max_levels(h, w), (w, h, n)
    for form, table in cases.FORMS.items():
        assert len(set(table)) == len(table), form


def sobel_and_window_sums(img):
    """numpy restatement of the Harris front end (oracle/oracle_harris.c) on the pixels that have all their neighbours:
    (gx, gy) of the 3 x 3 Sobel, and the 5 x 5 sums (a, b, d) of gx^2, gx gy, gy^2 — exact in int64, and `a` once more as a
    kernel that accumulated in fp32 would get it (window order, one rounding per addition)."""
    p = img.astype(np.int64)
    gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    rows, cols = gx.shape[0] - 4, gx.shape[1] - 4
    a, b, d = (np.zeros((rows, cols), np.int64) for _ in range(3))
    a_f32 = np.zeros((rows, cols), np.float32)
    for dr in range(5):
        for dc in range(5):
            x, y = gx[dr:dr + rows, dc:dc + cols], gy[dr:dr + rows, dc:dc + cols]
            a += x * x
            b += x * y
            d += y * y
            a_f32 = a_f32 + (x * x).astype(np.float32)  # (a single product is below 2^24: exact)
    return gx, gy, a, b, d, a_f32


@pytest.mark.parametrize("size", cases.HARRIS_SIZES, ids=lambda s: "%dx%d" % s)
def test_harris_images_reach_the_range_they_are_there_for(oracle, size):
    """What each image of the GPU Harris test delivers, asserted and not just written.  extremes and noise stay inside fp32's
    exact integers (every 5 x 5 sum below 2^24).  stripes has |g| == 1020, the end of the Sobel range, in x and in y, and sums of
    25 * 1020^2 > 2^24.  jitter passes 2^24 through odd partial sums, so an fp32 accumulation of the exact products differs
    from the integer sum at 45 % of the windows — and that changes the oracle's response bits, which the GPU test compares."""
    w, h = size
    top = {}
    for kind in cases.HARRIS_KINDS:
        gx, gy, a, b, d, a_f32 = sobel_and_window_sums(cases.image(kind, h, w))
        top[kind] = (int(np.abs(gx).max()), int(np.abs(gy).max()), int(a.max()), int(d.max()), int(np.abs(b).max()))
        print(f"{kind} {w} x {h}: max |gx| {top[kind][0]}, |gy| {top[kind][1]}, sum gx^2 {top[kind][2]}, gy^2 {top[kind][3]}, |gx gy| {top[kind][4]}; "
              f"fp32 accumulation of gx^2 differs at {100 * np.mean(a_f32.astype(np.int64) != a):.1f} % of the windows")
    assert top["extremes"][:2] == (510, 0)  # (rows r - 1 and r + 1 of the checkerboard are equal: no gy at all)
    assert max(top["extremes"][2:]) < 2 ** 24
    assert max(top["noise"][:2]) < 1020 and max(top["noise"][2:]) < 2 ** 24
    assert top["stripes"][:4] == (1020, 1020, 25 * 1020 ** 2, 25 * 1020 ** 2) and 25 * 1020 ** 2 > 2 ** 24
    assert min(top["jitter"][:2]) >= 996 and min(top["jitter"][2:4]) > 2 ** 24
    # jitter, at the centres Harris evaluates (11 pixels from the border): the float accumulation is wrong at many of them ...
    img = cases.image("jitter", h, w)
    _, _, a, b, d, a_f32 = sobel_and_window_sums(img)
    valid = (slice(11 - 3, h - 11 - 3), slice(11 - 3, w - 11 - 3))  # window sums start 3 pixels in
    wrong = a_f32.astype(np.int64)[valid] != a[valid]
    assert a[valid].shape == (h - 22, w - 22) and wrong.mean() >= 0.10
    # ... and the oracle's response is the one of the exact integer sums: restated here in fp32, bit for bit
    fa, fb, fd = a[valid].astype(np.float32), b[valid].astype(np.float32), d[valid].astype(np.float32)
    det = fa * fd - fb * fb
    tr = fa + fd
    exact = (det - (np.float32(0.04) * tr) * tr) * np.float32(1e-6)
    resp = oracle.harris_response(np.array(img))
    assert np.array_equal(resp[11:h - 11, 11:w - 11].view(np.uint32), exact.view(np.uint32))
    fa = a_f32[valid]
    det = fa * fd - fb * fb
    tr = fa + fd
    rounded = (det - (np.float32(0.04) * tr) * tr) * np.float32(1e-6)
    assert np.mean(rounded.view(np.uint32) != exact.view(np.uint32)) >= 0.05  # a float accumulation would be seen
