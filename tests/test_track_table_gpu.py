"""The track table's two entries on the device (device.track_table_retire_device, device.track_table_fill_device) against
the numpy restatement (tests/track_table_ref.py) at the slot counts, free-list lengths and values of tests/track_table_cases.py, whose
preconditions tests/test_track_table_cases_cpu.py establishes.  Every comparison is exact: integers, and float words as uint32.

Every array a kernel writes is the slice [GUARD : GUARD + n] of a larger allocation filled with a poison; the bands before and behind,
the free list behind n_free and every input must come back as they went in."""
import numpy as np
import pytest

from tests import track_table_cases as C
from tests import track_table_ref as R

pytestmark = pytest.mark.gpu

_DTYPES = {"ids": np.int64, "points": np.float32, "prev_points": np.float32, "status": np.uint8, "age": np.int32, "free_slots": np.int32,
           "n_live": np.int32, "n_free": np.int32, "next_id": np.int64}
_BITS = {np.dtype(np.float32): np.uint32}
_SCALARS = ("n_live", "n_free", "next_id")


def _bits(a):
    return a.view(_BITS.get(a.dtype, a.dtype))


class _DeviceTable:
    """The table of an R.Table on the device, inside guard bands, with a poisoned free list."""

    def __init__(self, dev, table):
        self.dev, self.n, self.full, self.view, self.sent, self.first = dev, table.n, {}, {}, {}, {}
        arrays = dict(table.tensors(), free_slots=None, n_free=None)  # the two that retire writes from nothing start as poison
        for name, a in arrays.items():
            count = 1 if name in _SCALARS else table.n
            first = 1 if name in _SCALARS else C.GUARD  # the one-element tensors sit in the middle of three elements
            host = np.empty((count + 2 * first,) + (() if a is None else a.shape[1:]), _DTYPES[name])
            _bits(host)[...] = np.array(C.GUARD_FILL[name]).astype(_bits(host).dtype)
            if a is not None:
                host[first:first + count] = a
            self.sent[name], self.first[name] = host.copy(), first
            self.full[name] = dev.torch.from_numpy(host).cuda()
            self.view[name] = self.full[name][first:first + count]
            assert self.view[name].is_contiguous() and (self.view[name].data_ptr() % 8 == 0 or name not in ("points", "prev_points"))
        self.free_slots = self.sent["free_slots"][C.GUARD:C.GUARD + table.n]  # as last read: the kernel writes n_free entries and no more

    def _inputs(self, **arrays):
        self.inputs = {k: (None if a is None else np.ascontiguousarray(a)) for k, a in arrays.items()}
        return {k: (None if a is None else self.dev.torch.from_numpy(a).cuda()) for k, a in self.inputs.items()}

    def retire(self, tracked_uv, tracked_status, back_uv=None, back_status=None, fb_threshold=0.0):
        v, torch = self.view, self.dev.torch
        t = self._inputs(tracked_uv=tracked_uv, tracked_status=tracked_status, back_uv=back_uv, back_status=back_status)
        torch.cuda.synchronize()
        self.dev.D.track_table_retire_device(self.dev.ctx, v["ids"], v["points"], v["prev_points"], v["status"], v["age"], v["n_live"], t["tracked_uv"],
                                             t["tracked_status"], v["free_slots"], v["n_free"], t["back_uv"], t["back_status"], fb_threshold)
        self.dev.ctx.synchronize()
        for k, a in self.inputs.items():
            assert a is None or np.array_equal(_bits(t[k].cpu().numpy()), _bits(a)), f"retire wrote its input {k}"

    def fill(self, pyramid, min_distance=C.FILL_MIN_DISTANCE, min_response=C.FILL_MIN_RESPONSE):
        v = self.view
        self.dev.torch.cuda.synchronize()
        self.dev.D.track_table_fill_device(self.dev.ctx, pyramid, min_distance, min_response, v["ids"], v["points"], v["prev_points"], v["status"], v["age"],
                                           v["n_live"], v["next_id"], v["free_slots"], v["n_free"])
        self.dev.ctx.synchronize()

    def read(self, what):
        """name -> the n entries the kernels own, after checking that nothing around them changed."""
        out = {}
        for name, full in self.full.items():
            got, sent, first = full.cpu().numpy(), self.sent[name], self.first[name]
            count = len(self.view[name])
            assert np.array_equal(_bits(got[:first]), _bits(sent[:first])), f"{what}: the band before {name} was written"
            assert np.array_equal(_bits(got[first + count:]), _bits(sent[first + count:])), f"{what}: the band behind {name} was written"
            out[name] = got[first:first + count]
        self.free_slots = out["free_slots"]
        return out


def _same(got, table, free, what, free_slots_before=None):
    """The seven tensors equal the restatement's; the free list is the restatement's, ascending, and behind its end what was there
    before the call (``free`` None after a fill: the caller holds the list to what retire wrote)."""
    for t, want in table.tensors().items():
        g, w = _bits(got[t]), _bits(want)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, t, g.dtype, g.shape)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, f"{what}: {t} differs in {bad.size} rows, first {bad[:5]}: got {got[t][bad[:5]]}, want {want[bad[:5]]}"
    if free is not None:
        n_free = int(got["n_free"][0])
        assert n_free == len(free), f"{what}: n_free {n_free}, want {len(free)}"
        listed = got["free_slots"][:n_free]
        assert np.array_equal(listed, np.array(free, np.int32)), f"{what}: the free list differs"
        assert (np.diff(listed) > 0).all(), f"{what}: the free list does not ascend"
        assert np.array_equal(got["free_slots"][n_free:], free_slots_before[n_free:]), f"{what}: free_slots was written behind n_free"


class _Device:
    def __init__(self, ftk):
        import torch
        from feature_tracker_amd import device as D
        self.torch, self.F, self.D = torch, ftk, D
        self.ctx = D.context_on_stream(torch.cuda.Stream())
        self._pyramid = None

    def pyramid(self):
        if self._pyramid is None:
            self._pyramid = self.F.ImagePyramid.from_host_levels([C.fill_image()], self.ctx)
        return self._pyramid


@pytest.fixture(scope="module")
def dev(ftk):
    return _Device(ftk)


def _retire_and_compare(dev, table, what, tracked_uv, tracked_status, back_uv=None, back_status=None, fb_threshold=0.0, on_device=None):
    """Retire on the device and in the restatement; returns (device table, what it holds, the restatement's free list)."""
    on_device = on_device or _DeviceTable(dev, table)
    empty_before = np.flatnonzero(table.ids < 0)
    held_before, free_slots_before = table.ids >= 0, on_device.free_slots.copy()
    on_device.retire(tracked_uv, tracked_status, back_uv, back_status, fb_threshold)
    free = table.retire(tracked_uv, tracked_status, back_uv, back_status, fb_threshold)
    got = on_device.read(what)
    _same(got, table, free, what, free_slots_before)
    retired_now = np.flatnonzero(held_before & (got["ids"] < 0))
    assert np.array_equal(got["free_slots"][:len(free)], np.union1d(empty_before, retired_now)), f"{what}: not the union of empty and retired"
    return on_device, got, free


@pytest.mark.parametrize("n", C.SIZES)
def test_retire_equals_the_restatement(dev, n):
    for k, pattern in enumerate(C.PATTERNS):
        table = C.state(n, k, C.held_mode(pattern))
        _retire_and_compare(dev, table, f"n {n}, {pattern}", C.tracked_points(n, k), C.outcome(table, pattern, k))


@pytest.mark.parametrize("n", C.FB_SIZES)
def test_retire_forward_backward(dev, n):
    for t in C.FB_THRESHOLDS:
        table = C.fb_state(n, 0)
        tracked_status, back_uv, back_status, _ = C.forward_backward(table, 0)
        _, got, free = _retire_and_compare(dev, table, f"n {n}, threshold {t}", C.tracked_points(n, 0), tracked_status, back_uv, back_status, t)
        if n > 2:
            assert (got["status"][got["ids"] < 0] == R.LARGE_RESIDUAL).any() and (got["ids"] >= 0).any() and len(free) > 0


def test_retire_hostile_values(dev):
    """NaN, +-inf, -0.0 and 1e30 from the tracker go into ``points`` bit for bit, for slots that stay and slots that go."""
    n = 2049
    uv = C.hostile_points(n, 0)
    for pattern in ("random", "every_status"):
        table = C.state(n, 0)
        held = table.ids >= 0
        _, got, _ = _retire_and_compare(dev, table, f"hostile, {pattern}", uv, C.outcome(table, pattern, 0))
        assert np.array_equal(_bits(got["points"])[held], _bits(uv)[held])
    table = C.fb_state(n, 0)
    tracked_status, back_uv, back_status, _ = C.forward_backward(table, 0)
    _retire_and_compare(dev, table, "hostile, forward-backward", uv, tracked_status, np.where(np.isfinite(uv), back_uv, uv), back_status, 1.0)


def _fill_and_compare(dev, table, on_device, what):
    points, mask = table.occupied()
    survivors = R.masked_survivors(C.fill_image(), C.FILL_MIN_DISTANCE, C.FILL_MIN_RESPONSE, points, mask)
    free, before, free_slots_before = list(table.free), {k: v.copy() for k, v in table.tensors().items()}, on_device.free_slots.copy()
    filled = table.fill(survivors)
    on_device.fill(dev.pyramid())
    got = on_device.read(what)
    _same(got, table, None, what)
    assert int(got["n_free"][0]) == len(free) and np.array_equal(got["free_slots"], free_slots_before), f"{what}: fill wrote the free list"
    assert filled == min(len(free), len(survivors)) and int(got["next_id"][0]) == int(before["next_id"][0]) + filled
    assert np.array_equal(got["ids"][free[:filled]], int(before["next_id"][0]) + np.arange(filled, dtype=np.int64))
    return survivors, filled, got


def test_fill_across_rank_tiles(dev):
    n = 2048
    probe, uv, st = C.fill_state(n, 0, 0)
    masked_count = len(R.masked_survivors(C.fill_image(), C.FILL_MIN_DISTANCE, C.FILL_MIN_RESPONSE, *probe.occupied()))
    counts = C.fill_free_counts(n, masked_count)
    assert masked_count > 3 * C.RANK_TILE and masked_count % C.RANK_TILE and counts[-1] == masked_count + 3
    for n_free in counts + [n]:
        table, uv, st = C.fill_state(n, n_free, 0)
        on_device, _, free = _retire_and_compare(dev, table, f"fill, n_free {n_free}: retire", uv, st)
        assert len(free) == n_free
        survivors, filled, _ = _fill_and_compare(dev, table, on_device, f"fill, n_free {n_free}")
        assert len(survivors) == (masked_count if n_free < n else len(C.fill_survivors())) and filled == min(n_free, len(survivors))


def test_fill_of_the_largest_table_when_every_slot_is_free(dev):
    """65 536 slots, none holds an id: the S survivors go into slots 0 .. S - 1, the slots behind stay empty and untouched."""
    n = C.MAX_SLOTS
    table = C.state(n, 0, "none")
    on_device, _, free = _retire_and_compare(dev, table, "fill at 65 536: retire", C.tracked_points(n, 0), C.outcome(table, "all_empty", 0))
    assert len(free) == n
    survivors, filled, got = _fill_and_compare(dev, table, on_device, "fill at 65 536")
    assert filled == len(survivors) == len(C.fill_survivors()) and int(got["n_live"][0]) == filled
    assert (got["ids"][filled:] == -1).all() and (_bits(got["points"][filled:]) == C.POISON_POINT_BITS).all() and (got["age"][filled:] == C.POISON_AGE).all()


@pytest.mark.parametrize("start", [2 ** 31 - 3, 2 ** 40 + 5])
def test_next_id_beyond_32_bits(dev, start):
    n, n_free = 1025, 400
    table, uv, st = C.fill_state(n, n_free, 1)
    table.next_id[0] = start
    on_device, _, free = _retire_and_compare(dev, table, f"next_id {start}: retire", uv, st)
    _, filled, got = _fill_and_compare(dev, table, on_device, f"next_id {start}")
    assert filled == n_free >= 300 and int(got["next_id"][0]) == start + n_free
    assert np.array_equal(got["ids"][free], start + np.arange(n_free, dtype=np.int64)) and got["ids"][free][-1] > 2 ** 31


def test_retire_then_fill_repeated(dev):
    """Five frames on one table that stays on the device: a stale free list or a count carried over between launches would show."""
    n = 2049
    table = C.state(n, 7)
    on_device, fills = _DeviceTable(dev, table), []
    for k, pattern in enumerate(("random", "all_dead", "alternating", "every_status", "random")):
        uv = C.hostile_points(n, k) if k == 3 else C.tracked_points(n, k)
        _retire_and_compare(dev, table, f"round {k}: retire ({pattern})", uv, C.outcome(table, pattern, 100 + k), on_device=on_device)
        n_free = len(table.free)
        survivors, filled, _ = _fill_and_compare(dev, table, on_device, f"round {k}: fill")
        fills.append((n_free, len(survivors), filled))
    assert any(f < s for f, s, _ in fills) and any(f > s for f, s, _ in fills) and all(done > C.RANK_TILE for _, _, done in fills), fills
