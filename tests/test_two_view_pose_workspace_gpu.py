"""``two_view_pose_device`` held to the sizes it declares, as tests/test_workspace_contract_gpu.py holds the other entries:
called directly on guarded memory (tests/guarded.py), the workspace exactly ``ceil(ftk_two_view_pose_workspace_bytes / 8)`` int64 words
and every output a payload of exactly its shape; twice on fresh arenas, all payloads 0x00 and all 0xFF, both results equal to the scalar
restatement bit for bit; no guard band written; the inputs other than status come back bit for bit."""
import numpy as np
import pytest

from tests import guarded as G
from tests import two_view_pose_ref as P

pytestmark = pytest.mark.gpu


def _run(ftk, name, fill):
    import torch
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    ref, cur, status = P.case(name)
    n = len(ref)
    specs = [("ref_uv", "float32", (n, 2), 0), ("cur_uv", "float32", (n, 2), 0), ("status", "uint8", (n,), 0),
             ("workspace", "int64", (-(-N.two_view_pose_workspace_bytes(n) // 8),), 0), ("pose", "float32", (7,), 0), ("points", "float32", (n, 3), 0),
             ("E", "float32", (3, 3), 0), ("n_front", "int32", (4,), 0), ("valid", "int32", (1,), 0), ("n_points", "int32", (1,), 0)]
    arena = G.Arena(specs, "cuda", fill=fill)
    inputs = dict(ref_uv=ref, cur_uv=cur, status=status)
    for key, array in inputs.items():
        arena.put(key, array)
    D.two_view_pose_device(ftk.default_context(), arena["ref_uv"], arena["cur_uv"], arena["status"], P.K, None, 1.0, 1.0, arena["workspace"], arena["pose"],
                           arena["points"], arena["E"], arena["n_front"], arena["valid"], arena["n_points"])
    torch.cuda.synchronize()
    host = arena.check()
    for key in ("ref_uv", "cur_uv"):
        assert arena.payload_bytes(key, host).tobytes() == np.ascontiguousarray(inputs[key]).tobytes(), f"the call changed its input {key}"
    r = P.Result()
    for key in P.OUTPUTS:
        setattr(r, key, arena[key].cpu().numpy())
    return r


@pytest.mark.parametrize("name", ["n7", "n9", "n64_half", "n256", "n257", "n1025", "hostile"])
def test_the_entry_in_its_declared_bytes(ftk, name):
    import ctypes as C
    from feature_tracker_amd import _native as N
    ref, cur, status = P.case(name)
    declared = C.c_int64()
    assert N.lib().ftk_two_view_pose_workspace_bytes(len(ref), C.byref(declared)) == 0
    assert declared.value == N.two_view_pose_workspace_bytes(len(ref))
    want = P.solve(ref, cur, status)
    for fill in (G.ZEROS, G.ONES):
        assert P.same_results(_run(ftk, name, fill), want) == [], (name, hex(fill))
