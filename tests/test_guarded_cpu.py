"""tests/guarded.py on CPU tensors: a clean arena passes, one byte written right in front of a payload, right behind one, or at the far
end of a band is reported with the neighbours' names and the offset, the payload views have exactly the asked size, type and alignment,
and the two builds of a poison pair differ in payload bytes only."""
import numpy as np
import pytest

from tests import guarded as G

# an odd byte count, a count that is no multiple of the alignment, one larger than the least band, one element
SPECS = [("status", "uint8", (257,), 0x11), ("uv", "float32", (300, 2), 0x22), ("workspace", "int64", (1031,), 0x33), ("count", "int32", (1,), 0x44),
         ("models", "float32", (2, 65, 9), 0x55)]


def _arena(**kw):
    torch = pytest.importorskip("torch")
    return torch, G.Arena(SPECS, "cpu", **kw)


def test_a_clean_arena_passes_and_its_layout_is_as_documented():
    torch, arena = _arena()
    host = arena.check()
    assert host.shape == (arena.total,) and arena.buf.data_ptr() % G.ALIGN == 0
    end = 0
    for k, (name, dtype, shape, fill) in enumerate(SPECS):
        a, b = arena.span(name)
        nbytes = int(np.prod(shape)) * torch.empty(0, dtype=getattr(torch, dtype)).element_size()
        assert b - a == nbytes and a % G.ALIGN == 0
        # the band in front is at least 4096 bytes and at least as large as both neighbours (none of them reaches the 1 MiB cap)
        assert a - end >= max(G.MIN_GUARD, nbytes, 0 if k == 0 else arena.span(SPECS[k - 1][0])[1] - arena.span(SPECS[k - 1][0])[0])
        assert (host[end:a] == G.GUARD_BYTE).all() and (host[a:b] == fill).all()
        end = b
    assert arena.total - end >= max(G.MIN_GUARD, nbytes) and (host[end:] == G.GUARD_BYTE).all()


def test_the_band_follows_a_large_neighbour_up_to_the_cap():
    torch, _ = _arena()
    arena = G.Arena([("small", "uint8", (3,), 1), ("plane", "uint8", (G.MAX_GUARD + 4096,), 2), ("tail", "int32", (5,), 3)], "cpu")
    (_, small_end), (plane_at, plane_end), (tail_at, tail_end) = arena.span("small"), arena.span("plane"), arena.span("tail")
    assert G.MAX_GUARD <= plane_at - small_end < G.MAX_GUARD + G.ALIGN and G.MAX_GUARD <= tail_at - plane_end < G.MAX_GUARD + G.ALIGN
    assert arena.total - tail_end == G.MIN_GUARD
    arena.check()


def test_payload_views_have_the_exact_size_type_and_alignment():
    torch, arena = _arena()
    for name, dtype, shape, fill in SPECS:
        view = arena[name]
        assert view.dtype == getattr(torch, dtype) and tuple(view.shape) == shape and view.numel() == int(np.prod(shape))
        assert view.is_contiguous() and view.data_ptr() % G.ALIGN == 0
        assert view.data_ptr() - arena.buf.data_ptr() == arena.span(name)[0]
        assert (view.view(torch.uint8) == fill).all()
    # a view writes the arena: it is no copy
    arena["count"][0] = 0x01020304
    assert arena.payload_bytes("count").tolist() == [4, 3, 2, 1]
    arena.check()


@pytest.mark.parametrize("name", [s[0] for s in SPECS])
def test_one_byte_right_in_front_of_a_payload_is_reported(name):
    torch, arena = _arena()
    a, _ = arena.span(name)
    arena.buf[a - 1] = 0
    with pytest.raises(G.GuardDamaged) as e:
        arena.check()
    k = [s[0] for s in SPECS].index(name)
    assert e.value.after == name and e.value.before == (SPECS[k - 1][0] if k else None)
    assert e.value.first == e.value.last == a - 1 and e.value.ahead_of_after == 1 and e.value.damaged == 1
    assert f"1 bytes ahead of the start of '{name}'" in str(e.value)


@pytest.mark.parametrize("name", [s[0] for s in SPECS])
def test_one_byte_right_behind_a_payload_is_reported(name):
    torch, arena = _arena()
    _, b = arena.span(name)
    arena.buf[b] = 0xFF
    with pytest.raises(G.GuardDamaged) as e:
        arena.check()
    k = [s[0] for s in SPECS].index(name)
    assert e.value.before == name and e.value.after == (SPECS[k + 1][0] if k + 1 < len(SPECS) else None)
    assert e.value.first == e.value.last == b and e.value.past_before == 0
    assert f"starts 0 bytes past the end of '{name}'" in str(e.value)


def test_one_byte_at_the_far_end_of_a_band_is_reported():
    # the last byte of the arena, the first byte of the arena, and the last byte of an inner band seen from the payload in front of it
    for where, before, after in (("end", "models", None), ("start", None, "status"), ("inner", "uv", "workspace")):
        torch, arena = _arena()
        at = {"end": arena.total - 1, "start": 0, "inner": arena.span("workspace")[0] - 1}[where]
        arena.buf[at] ^= 0x01  # one bit
        with pytest.raises(G.GuardDamaged) as e:
            arena.check()
        assert (e.value.before, e.value.after, e.value.first, e.value.last) == (before, after, at, at)
        if before is not None:
            assert e.value.past_before == at - arena.span(before)[1]


def test_a_run_of_damage_reports_its_first_and_last_byte():
    torch, arena = _arena()
    _, b = arena.span("uv")
    arena.buf[b:b + 2400].view(torch.float32)[:] = 1.0  # a whole row block past the end
    with pytest.raises(G.GuardDamaged) as e:
        arena.check()
    assert (e.value.before, e.value.after, e.value.first, e.value.last) == ("uv", "workspace", b, b + 2399)


def test_a_poison_pair_differs_in_payload_bytes_only():
    torch = pytest.importorskip("torch")
    zeros, ones = G.poison_pair(SPECS, "cpu")
    a, b = zeros.check(), ones.check()
    assert zeros.spans == ones.spans and zeros.total == ones.total
    mask = zeros.payload_mask()
    assert mask.sum() == sum(e - s for s, e in zeros.spans.values())
    assert (a[mask] == G.ZEROS).all() and (b[mask] == G.ONES).all() and np.array_equal(a[~mask], b[~mask]) and (a[~mask] == G.GUARD_BYTE).all()
    # what the all-ones fill reads as
    assert torch.isnan(ones["uv"]).all() and (ones["count"] == -1).all() and (ones["workspace"] == -1).all() and (ones["status"] == 255).all()
    assert not zeros["uv"].any() and not zeros["workspace"].any()


def test_put_and_same_bytes():
    torch, arena = _arena()
    uv = np.random.default_rng(0).standard_normal((300, 2)).astype(np.float32)
    uv[3, 1] = np.nan
    view = arena.put("uv", uv)
    assert view.data_ptr() == arena["uv"].data_ptr() and G.same_bytes(arena["uv"], uv)
    arena["uv"].view(torch.int32)[3, 1] ^= 1  # another NaN: not the same bytes
    assert not G.same_bytes(arena["uv"], uv)
    arena.check()
