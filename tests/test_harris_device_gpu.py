"""Masked Harris detection on the device (FeaturePointHarrisDetector.detect_device, ftk_harris_detect_device) against the
numpy restatement (tests/track_table_ref.py): rows, the zeros behind them and the count, exactly."""
import os

import numpy as np
import pytest

from feature_tracker_amd import synth
from tests import track_table_ref as R

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "optical_flow")
SIZES = [(23, 23), (24, 40), (64, 48), (333, 251)]  # width x height; 23 x 23 has one valid centre
DISTANCES = [1, 2, 9, 25]
MIN_RESPONSE = 40.0


def _scene(width, height):
    return np.ascontiguousarray(synth.make_image_pair(max(width, 32), max(height, 32), (0.0, 0.0))[0][:height, :width])


def occupied_sets(image, distance):
    """name -> (points [n, 2] float32, flags [n] uint8 or None)."""
    rows, cols = image.shape
    rs = np.random.RandomState(rows * 1000 + cols + distance)
    strongest = R.masked_survivors(image, distance, MIN_RESPONSE)
    sets = {"none": (None, None), "border_band": (np.array([[3.0, 5.0]], np.float32), None)}
    if len(strongest):
        sets["on_the_strongest"] = (strongest[:1].copy(), None)
    dense = np.stack([rs.uniform(-2, cols + 2, 200), rs.uniform(-2, rows + 2, 200)], axis=1).astype(np.float32)
    sets["dense_random"] = (dense, (rs.uniform(size=200) < 0.7).astype(np.uint8))
    sets["all_flags_zero"] = (dense, np.zeros(200, np.uint8))
    edge = np.array([[cols - 1, rows // 2], [cols - 1 + 0.5, rows // 2 + 0.5], [cols // 2 + 0.5, rows // 2 - 0.5], [cols // 2 - 1.5, 11.5],
                     [11.49999, rows - 12 + 0.5]], np.float32)
    sets["last_column_and_half_pixels"] = (edge, None)
    return sets


class _Device:
    def __init__(self, ftk):
        import torch
        from feature_tracker_amd import device as D
        self.torch, self.F = torch, ftk
        self.ctx = D.context_on_stream(torch.cuda.Stream())

    def detect(self, pyramid, distance, max_count, points, flags):
        torch = self.torch
        det = self.F.FeaturePointHarrisDetector(self.ctx)
        det.options().kMinFeatureDistance, det.options().kMinValidResponse = distance, MIN_RESPONSE
        occ = None if points is None else torch.from_numpy(points).cuda()
        msk = None if flags is None else torch.from_numpy(flags).cuda()
        torch.cuda.synchronize()
        uv, count = det.detect_device(pyramid, max_count, occ, msk)
        self.ctx.synchronize()
        return uv.cpu().numpy(), int(count.cpu().numpy()[0])


@pytest.fixture(scope="module")
def dev(ftk):
    return _Device(ftk)


def _check_image(dev, image, distance):
    pyramid = dev.F.ImagePyramid.from_host_levels([image], dev.ctx)
    for name, (points, flags) in occupied_sets(image, distance).items():
        survivors = R.masked_survivors(image, distance, MIN_RESPONSE, points, flags)
        S = len(survivors)
        for max_count in sorted({max(S - 1, 0), S, S + 3, 1}):
            want = np.zeros((max_count, 2), np.float32)
            want[:min(S, max_count)] = survivors[:max_count]
            uv, count = dev.detect(pyramid, distance, max_count, points, flags)
            assert count == min(S, max_count), (name, max_count, count, S)
            assert np.array_equal(uv, want), (name, max_count)
    return pyramid


@pytest.mark.parametrize("distance", DISTANCES)
@pytest.mark.parametrize("width,height", SIZES)
def test_detection_equals_the_restatement(dev, width, height, distance):
    image = _scene(width, height)
    if R.survivor_bound(height, width, distance) > 65536:
        pyramid = dev.F.ImagePyramid.from_host_levels([image], dev.ctx)
        with pytest.raises(ValueError, match="FTK_HARRIS_DEVICE_MAX_SURVIVORS"):
            dev.detect(pyramid, distance, 10, None, None)
        return
    pyramid = _check_image(dev, image, distance)
    # with no occupied point: FeaturePointHarrisDetector.DetectGoodFeatures
    det = dev.F.FeaturePointHarrisDetector(dev.ctx)
    det.options().kMinFeatureDistance, det.options().kMinValidResponse = distance, MIN_RESPONSE
    ok, host_uv = det.DetectGoodFeatures(pyramid, 50)
    uv, count = dev.detect(pyramid, distance, 50, None, None)
    assert ok and count == len(host_uv) and np.array_equal(uv[:count], host_uv)


def test_example_image(dev):
    from PIL import Image
    _check_image(dev, np.array(Image.open(os.path.join(DATA, "ref_image.png"))), 25)


def test_identical_corners_break_the_tie_by_pixel_index(dev):
    """Two identical bright squares: their corners have identical responses.  Within one window the smaller pixel index wins; apart, both
    survive and the smaller index comes first."""
    image = np.full((64, 96), 20, np.uint8)
    image[20:30, 20:30] = 220
    image[20:30, 50:60] = 220
    resp = R.oracle_lib.harris_response(image)
    assert resp[20, 20] == resp[20, 50] and resp[20, 20] > MIN_RESPONSE
    for distance in (3, 45):
        survivors = R.masked_survivors(image, distance, MIN_RESPONSE)
        pyramid = dev.F.ImagePyramid.from_host_levels([image], dev.ctx)
        uv, count = dev.detect(pyramid, distance, 64, None, None)
        assert count == len(survivors) and np.array_equal(uv[:count], survivors) and not uv[count:].any()
        resp_of = resp[survivors[:, 1].astype(int), survivors[:, 0].astype(int)]
        ties = np.flatnonzero(resp_of[1:] == resp_of[:-1])
        if distance == 3:
            assert ties.size > 0  # equal responses next to each other in the order: pixel index ascending
        index = survivors[:, 1].astype(int) * 96 + survivors[:, 0].astype(int)
        assert (index[ties + 1] > index[ties]).all()
