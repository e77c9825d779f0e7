"""ftk_match_table_query_device and ftk_match_table_update_device against the restatement (tests/match_table_ref.py), bit for bit on
every output including the rows behind the counts: the wave, workgroup and four-per-thread edges of the scan in n_slots and K, scalar
and 16-byte descriptor rows, a descriptor base that is only 4-byte aligned, the table occupancies, the hand-written scenarios and the
three forms of cur_count."""
import numpy as np
import pytest

from tests import match_table_cases as Cases
from tests import match_table_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EDGES = (1, 63, 64, 65, 1023, 1024, 1025, 4096)
DIMS = (1, 3, 4, 65, 256)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def descriptor_tensor(array, offset_floats=0):
    """A contiguous CUDA [rows, D] tensor of ``array`` whose base lies ``offset_floats`` floats behind a 256-byte boundary."""
    flat = torch.zeros(array.size + offset_floats, dtype=torch.float32, device="cuda")
    view = flat[offset_floats:].view(array.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(array)))
    return view


def on_device(table, offset_floats=0):
    t = {k: torch.from_numpy(v.copy()).cuda() for k, v in table.tensors().items() if k != "descriptors"}
    t["descriptors"] = descriptor_tensor(table.descriptors, offset_floats)
    return t


def check_query(ctx, table, offset_floats=0):
    from feature_tracker_amd import device as D
    n, d = table.n, table.dim
    t = on_device(table, offset_floats)
    q_uv = torch.full((n, 2), 7.0, device="cuda")
    q_desc = descriptor_tensor(np.full((n, d), 7.0, np.float32), offset_floats)
    q_slot = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    q_count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    D.match_table_query_device(ctx, t["ids"], t["points"], t["descriptors"], q_uv, q_desc, q_slot, q_count)
    want = table.query()
    for name, got, ref in zip(("q_uv", "q_desc", "q_slot", "q_count"), (q_uv, q_desc, q_slot, q_count), want):
        assert same_bits(got.cpu().numpy(), ref), name
    for k, v in table.tensors().items():  # the table is not written
        assert same_bits(t[k].cpu().numpy(), v), k
    return q_slot, q_count


def check_update(ctx, table, index, status, uv, desc, cur_count, max_lost, q_count=None, offset_floats=0, with_cur_slot=True):
    """The device entry on a copy of ``table`` against ``table.update`` (which moves ``table`` on)."""
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    n, d, k = table.n, table.dim, uv.shape[0]
    t = on_device(table, offset_floats)
    _, _, q_slot, nq = table.query()
    q_count = int(nq[0]) if q_count is None else q_count
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    count_t = None if cur_count is None else torch.tensor([cur_count], dtype=torch.int32, device="cuda")
    workspace = torch.full((-(-N.match_table_workspace_bytes(n, k, d) // 8),), -1, dtype=torch.int64, device="cuda")
    cur_slot = torch.full((k,), 77, dtype=torch.int32, device="cuda") if with_cur_slot else None
    D.match_table_update_device(ctx, t["ids"], t["points"], t["prev_points"], t["descriptors"], t["status"], t["age"], t["lost"], t["n_live"], t["next_id"],
                                dev(q_slot), torch.tensor([q_count], dtype=torch.int32, device="cuda"), dev(index), dev(status), dev(uv),
                                descriptor_tensor(desc, offset_floats), count_t, max_lost, workspace, cur_slot)
    want_slot = table.update(q_slot, q_count, index, status, uv, desc, cur_count, max_lost)
    for name, v in table.tensors().items():
        assert same_bits(t[name].cpu().numpy(), v), name
    got_slot = cur_slot if with_cur_slot else workspace.view(torch.int32)[:k]
    assert same_bits(got_slot.cpu().numpy(), want_slot), "cur_slot"


def occupied(n, d, kind, rng):
    live = {"empty": [], "full": range(n), "alternating": range(0, n, 2), "last": [n - 1]}[kind]
    table = Cases.seeded(n, d, live)
    table.descriptors[list(live)] = rng.standard_normal((len(list(live)), d)).astype(np.float32)
    table.lost[list(live)] = rng.integers(0, 3, len(list(live)))
    return table


@pytest.mark.parametrize("n, k", list(zip(EDGES, reversed(EDGES))) + [(4096, 4096)])
def test_scan_edges(gpu_ctx, n, k):
    rng = np.random.default_rng(n * 7 + k)
    d = DIMS[EDGES.index(n) % len(DIMS)] if (n, k) != (4096, 4096) else 4
    table = R.Table(n, d)
    for step in range(3):  # from empty: everything admitted, then two frames of hits, misses, collisions and rejections
        check_query(gpu_ctx, table)
        q_slot, nq, index, status, uv, desc = Cases.random_frame(rng, table, k)
        check_update(gpu_ctx, table, index, status, uv, desc, None, step % 2, with_cur_slot=step != 1)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("kind", ["empty", "full", "alternating", "last"])
def test_occupancies_and_widths(gpu_ctx, d, kind):
    rng = np.random.default_rng(d * 5 + len(kind))
    table = occupied(1025, d, kind, rng)
    check_query(gpu_ctx, table)
    _, _, index, status, uv, desc = Cases.random_frame(rng, table, 1023)
    check_update(gpu_ctx, table, index, status, uv, desc, 1000, 1)
    check_query(gpu_ctx, table)


@pytest.mark.parametrize("d", [4, 256])
def test_a_descriptor_base_that_is_only_4_byte_aligned(gpu_ctx, d):
    rng = np.random.default_rng(d)
    table = occupied(130, d, "alternating", rng)
    check_query(gpu_ctx, table, offset_floats=1)
    _, _, index, status, uv, desc = Cases.random_frame(rng, table, 67)
    check_update(gpu_ctx, table, index, status, uv, desc, None, 0, offset_floats=1)


@pytest.mark.parametrize("name", Cases.SCENARIOS)
def test_hand_written_scenarios(gpu_ctx, name):
    table, index, status, k, cur_count, q_count, max_lost = Cases.scenario(name)
    check_query(gpu_ctx, table)
    uv, desc = Cases.cur_rows(k, table.dim)
    check_update(gpu_ctx, table, index, status, uv, desc, cur_count, max_lost, q_count=q_count)


@pytest.mark.parametrize("cur_count", [None, 0, 65])
def test_cur_count_forms(gpu_ctx, cur_count):
    rng = np.random.default_rng(3)
    table = occupied(64, 4, "alternating", rng)
    _, _, index, status, uv, desc = Cases.random_frame(rng, table, 65)
    check_update(gpu_ctx, table, index, status, uv, desc, cur_count, 0)


def test_the_entries_refuse_before_any_launch(gpu_ctx):
    import ctypes as C
    from feature_tracker_amd import _native as N
    lib, h = N.lib(), gpu_ctx.handle
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    at = lambda k: C.c_void_p(buf.data_ptr() + 256 * k)  # noqa: E731
    q = lambda n=4, d=4, ptrs=None: lib.ftk_match_table_query_device(h, None, n, d, *(ptrs or [at(i) for i in range(7)]))  # noqa: E731
    assert q(0) == -1 and q(4097) == -1 and q(4, 0) == -1 and q(4, 1025) == -1
    assert q(ptrs=[at(0), at(1), at(2), at(3), at(4), at(5), None]) == -1
    assert q(ptrs=[at(0), at(1), at(2), at(3), at(4), at(5), at(0)]) == -1  # an alias
    assert q(ptrs=[at(0), C.c_void_p(buf.data_ptr() + 260), at(2), at(3), at(4), at(5), at(6)]) == -1  # points 4-byte aligned
    assert b"alias" in lib.ftk_last_error(h) or b"aligned" in lib.ftk_last_error(h)

    def u(n=4, d=4, k=4, max_lost=0, ptrs=None, count=at(15), ws=at(16), slot=at(17)):
        ptrs = ptrs or [at(i) for i in range(15)]
        return lib.ftk_match_table_update_device(h, None, n, d, *ptrs, k, count, max_lost, ws, slot)

    assert u(0) == -1 and u(4097) == -1 and u(d=0) == -1 and u(d=1025) == -1 and u(k=0) == -1 and u(k=4097) == -1 and u(max_lost=-1) == -1
    assert u(ws=None) == -1 and u(ptrs=[at(i) for i in range(14)] + [None]) == -1
    assert u(slot=at(3)) == -1 and u(count=at(16)) == -1 and u(ptrs=[at(i) for i in range(14)] + [at(2)]) == -1  # aliases
    assert u(ws=C.c_void_p(buf.data_ptr() + 16 * 256 + 8)) == -1  # the workspace 8-byte aligned
    assert q() == 0 and u() == 0 and u(count=None, slot=None) == 0
    torch.cuda.synchronize()
