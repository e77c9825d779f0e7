"""scripts/benchlib.py's two timing loops on the device, on a 1 024-element float32 add.  No time is asserted: only that every figure is a
finite positive number and that the percentiles are ordered."""
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from scripts import benchlib  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def adds():
    import torch

    x = [torch.ones(1024, dtype=torch.float32, device="cuda") for _ in range(3)]
    return torch, [lambda t=t: t + t for t in x]


def test_wall_times_on_the_device(adds):
    torch, (fn, _, _) = adds
    times = benchlib.wall_times(torch, fn, 5, 2)
    assert len(times) == 5 and all(math.isfinite(t) and t > 0 for t in times)


@pytest.mark.parametrize("n_fns,calls,warmup", [(1, 5, 2), (3, 6, 1)])
def test_event_times_on_the_device(adds, n_fns, calls, warmup):
    torch, fns = adds
    median, p10, p90 = benchlib.event_times(torch, fns[:n_fns], calls, warmup)
    assert all(math.isfinite(v) and v > 0 for v in (median, p10, p90))
    assert p10 <= median <= p90
