"""The staging layouts of the host-buffer entry points (csrc/ftk_layout.h) on the CPU, through host/build/layout_cli: for the sequence
of take() calls every entry makes, each offset, each copy span and the total equal the formulas the entries spelled out by hand
before the layout type existed (restated below from that source: columns of align_up(..., 256) and sums of them).  Three tails were
irregular there (a bare `+ 256`, an unpadded status array); as slots of their own they may only grow, by at most 256 bytes.
The 16-byte flavour of the same class, which lays out the caller-owned workspaces (csrc/*_plan.h), is held to the take rule itself at
the end of the file; the workspaces' own byte formulas are restated in the *_args_cpu.py tests."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "feature_tracker_amd", "host", "build", "layout_cli")

SIZE_MAX = 2 ** 64 - 1
COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 16384, 16385)
# (row_bytes, dev_row_bytes) of the matchers: 96-bit descriptors are padded to 4 words on the host, 256-bit ones are not; 128 floats
ROWS = ((12, 16), (32, 32), (512, 512))


def al(x):
    return (x + 255) // 256 * 256


def cli(lines):
    assert os.path.exists(EXE), "host layer not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in r.stdout.splitlines()]
    assert len(out) == sum(1 for l in lines if l not in ("new", "new16"))
    return out


def walk(takes, spans=()):
    """(offsets, spans, total) of one layout: takes = [(elem_bytes, count)], spans = [(first slot, last slot)]."""
    out = cli(["new"] + [f"take {e} {c}" for e, c in takes] + [f"span {i} {j}" for i, j in spans] + ["total"])
    slots, sp, total = out[:len(takes)], out[len(takes):-1], out[-1]
    assert all(s["ok"] == 1 for s in slots) and total["ok"] == 1
    assert all(s["offset"] % 256 == 0 for s in slots)
    assert [s["size"] for s in slots] == [e * c for e, c in takes]  # the payload, unpadded
    return [s["offset"] for s in slots], [s["span"] for s in sp], total["total"]


@pytest.mark.parametrize("n", COUNTS)
def test_klt_track(n):
    uv, st, it = al(4 * 2 * n), al(n), al(4 * n)  # ftk_klt_track (and ftk_klt_track_sharded's stage block)
    offsets, spans, total = walk([(4, 2 * n), (4, 2 * n), (1, n), (4, n)], [(0, 2), (1, 2), (1, 3)])
    assert offsets == [0, uv, 2 * uv, 2 * uv + st]
    assert total == 2 * uv + st + it
    assert spans == [2 * uv + st, uv + st, uv + st + it]  # the H2D; the D2H without and with iters


@pytest.mark.parametrize("row_bytes,dev_row_bytes", ROWS)
@pytest.mark.parametrize("with_pred", (False, True))
def test_staged_match(row_bytes, dev_row_bytes, with_pred):
    for n_ref in COUNTS:
        for n_cur in (1, 33, 65, n_ref):
            ref, cur = al(dev_row_bytes * n_ref), al(dev_row_bytes * n_cur)
            pred, cuv = (al(4 * 2 * n_ref), al(4 * 2 * n_cur)) if with_pred else (0, 0)
            idx_at = ref + cur + pred + cuv
            offsets, spans, total = walk([(1, dev_row_bytes * n_ref), (1, dev_row_bytes * n_cur), (4, 2 * n_ref if with_pred else 0),
                                          (4, 2 * n_cur if with_pred else 0), (4, n_ref)], [(0, 1)])
            assert offsets == [0, ref, ref + cur, ref + cur + pred, idx_at]
            assert total == idx_at + al(4 * n_ref)  # in_bytes: the one H2D
            assert spans == [ref + cur]             # the memset of the padded rows


@pytest.mark.parametrize("n_bits", (96, 256))
def test_brief_compute(n_bits):
    n_words = (n_bits + 31) // 32
    for n in COUNTS:
        uv, w = al(4 * 2 * n), al(4 * n_words * n)
        offsets, _, total = walk([(4, 2 * n), (4, n_words * n)])
        assert offsets == [0, uv]
        assert total == uv + w


@pytest.mark.parametrize("px", COUNTS + (120 * 160,))
def test_harris(px):
    capacity = px
    g, f, k, l = al(2 * px), al(4 * px), al(8 * px), al(8 * capacity)
    offsets, _, total = walk([(2, px), (2, px), (4, px), (8, px), (8, px), (8, px), (8, capacity), (4, 1)])
    assert offsets == [0, g, 2 * g, 2 * g + f, 2 * g + f + k, 2 * g + f + 2 * k, 2 * g + f + 3 * k, 2 * g + f + 3 * k + l]
    old = 2 * g + f + 3 * k + l + 256  # the counter's `+ 256`
    assert old <= total <= old + 256


@pytest.mark.parametrize("ref_px,cur_px", [(n, n) for n in COUNTS if n] + [(48 * 64, 48 * 64), (129, 65), (65, 129)])
def test_dense_setup(ref_px, cur_px):
    mom_ref, mom_cur, plane = al(2 * 16 * ref_px), al(2 * 16 * cur_px), al(4 * ref_px)
    offsets, _, total = walk([(16, 2 * ref_px), (16, 2 * cur_px)] + [(4, ref_px)] * 4)
    assert offsets == [0, mom_ref] + [mom_ref + mom_cur + i * plane for i in range(4)]
    assert total == mom_ref + mom_cur + 4 * plane
    # the host entries' [flow_r | flow_c], in the scratch and the pinned block
    offsets, _, total = walk([(4, ref_px), (4, ref_px)])
    assert offsets == [0, plane] and total == 2 * plane


@pytest.mark.parametrize("n", COUNTS)
def test_direct_track(n):
    pts, uv, st = al(4 * 3 * n), al(4 * 2 * n), al(n)
    offsets, _, total = walk([(4, 3 * n), (4, 2 * n), (4, 2 * n), (1, n), (4, 7), (4, 1)])
    assert offsets == [0, pts, pts + uv, pts + 2 * uv, pts + 2 * uv + st, pts + 2 * uv + st + 256]
    assert total == pts + 2 * uv + st + 256 + 256


@pytest.mark.parametrize("n", COUNTS)
def test_irregular_tails(n):
    # ftk_extract_extend_patch: [patch | valid] + 256 for the counter
    patch, valid = al(4 * n), al(n)
    offsets, _, total = walk([(4, n), (1, n), (4, 1)])
    assert offsets == [0, patch, patch + valid]
    assert patch + valid + 256 <= total <= patch + valid + 256 + 256
    # ftk_nn.cpp run_nn_host: [input | index] and an unpadded status tail, with and without input (an empty match list)
    for in_bytes in (0, 16 * n, 4 * n * 33):
        in_pad, idx_pad = al(in_bytes), al(4 * n)
        offsets, _, total = walk([(1, in_bytes), (4, n), (1, n)])
        assert offsets == [0, in_pad, in_pad + idx_pad]
        assert in_pad + idx_pad + n <= total <= in_pad + idx_pad + n + 256
    # ftk_ldlt6_solve
    a, b = al(4 * 36 * n), al(4 * 6 * n)
    offsets, _, total = walk([(4, 36 * n), (4, 6 * n), (4, 6 * n)])
    assert offsets == [0, a, a + b] and total == a + 2 * b


def test_a_wrapping_count_voids_the_layout():
    """A count whose padded byte size would wrap size_t: the flag drops and stays down, and bytes() is never a small number."""
    last_good = (SIZE_MAX - 255) // 4  # 4 * count == 2^64 - 256: its padded end is still a size_t
    out = cli(["new", f"take 4 {last_good}", "total"])
    assert out[0]["ok"] == 1 and out[1] == {"total": 4 * last_good, "ok": 1}
    for lines in (["new", f"take 4 {last_good + 1}", "total"],
                  ["new", f"take 4 {SIZE_MAX // 4}", "total"],                # 2^64 - 4 bytes: only the padding wraps
                  ["new", f"take 4 {SIZE_MAX // 4 + 2}", "total"],            # the product itself wraps to 4
                  ["new", "take 4 130", f"take 8 {SIZE_MAX // 8 - 64}", "total"],  # fits alone, not behind the first slot
                  ["new", f"take 16 {SIZE_MAX // 16 + 1}", "take 1 1", "total"]):  # and nothing taken later revives it
        out = cli(lines)
        assert out[-2]["ok"] == 0 and out[-1] == {"total": SIZE_MAX, "ok": 0}, lines


def up16(x):
    return (x + 15) // 16 * 16


def test_sixteen_byte_slots_in_call_order():
    """Every slot on the next 16-byte boundary, in call order; the payload unpadded, the padded size the payload rounded up to 16 bytes,
    for byte sizes that are multiples of 16 (0 aside), one below, one above, and far from one."""
    takes = [(4, 1), (16, 7), (4, 4), (4, 5), (1, 15), (1, 16), (1, 17), (8, 2), (8, 3), (2, 8), (2, 9), (4, 45 * 257), (1, 4096 + 1), (4, 32)]
    out = cli(["new16"] + [f"take {e} {c}" for e, c in takes] + ["span 1 3", "span 0 13", "total"])
    end = 0
    for (e, c), s in zip(takes, out):
        assert s == {"offset": end, "size": e * c, "padded": up16(e * c), "ok": 1}, (e, c)
        assert s["offset"] % 16 == 0 and 0 <= s["padded"] - s["size"] < 16
        end += up16(e * c)
    assert out[-3] == {"span": up16(16 * 7) + 16 + up16(4 * 5)} and out[-2] == {"span": end}
    assert out[-1] == {"total": end, "ok": 1}
    assert sum(1 for e, c in takes if e * c % 16 == 0) >= 4 and sum(1 for e, c in takes if e * c % 16 != 0) >= 4


def test_a_sixteen_byte_slot_of_count_zero_occupies_nothing():
    out = cli(["new16", "take 4 0", "take 8 3", "take 1 0", "take 16 0", "take 4 1", "take 8 0", "total"])
    assert [s["offset"] for s in out[:-1]] == [0, 0, 32, 32, 32, 48]  # an empty slot reports the running end
    assert [s["padded"] for s in out[:-1]] == [0, 32, 0, 0, 16, 0] and [s["size"] for s in out[:-1]] == [0, 24, 0, 0, 4, 0]
    assert all(s["ok"] == 1 for s in out) and out[-1]["total"] == 48


def test_a_wrapping_count_voids_the_sixteen_byte_layout():
    last_good = (SIZE_MAX - 15) // 4  # 4 * count == 2^64 - 16: its padded end is still a size_t
    out = cli(["new16", f"take 4 {last_good}", "total"])
    assert out[0]["ok"] == 1 and out[1] == {"total": 4 * last_good, "ok": 1}
    for lines in (["new16", f"take 4 {last_good + 1}", "total"],                     # 2^64 - 12 bytes: only the padding wraps
                  ["new16", f"take 4 {SIZE_MAX // 4 + 2}", "total"],                 # the product itself wraps to 4
                  ["new16", "take 4 5", f"take 8 {SIZE_MAX // 8 - 3}", "total"],     # fits alone, not behind the first slot
                  ["new16", f"take 16 {SIZE_MAX // 16 + 1}", "take 1 1", "total"]):  # and nothing taken later revives it
        out = cli(lines)
        assert out[-2]["ok"] == 0 and out[-1] == {"total": SIZE_MAX, "ok": 0}, lines
    # a 256-byte layout made after a 16-byte one is a 256-byte layout again
    out = cli(["new16", "take 1 1", "new", "take 1 1", "take 1 1", "total"])
    assert [s["offset"] for s in out[:3]] == [0, 0, 256] and out[-1] == {"total": 512, "ok": 1}
