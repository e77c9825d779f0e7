"""``pnp_ransac_sampled_device`` held to the sizes it declares, as tests/test_pnp_workspace_gpu.py holds
``pnp_ransac_device``: called directly on guarded memory (tests/guarded.py), the workspace exactly
``ceil(ftk_pnp_ransac_workspace_bytes / 8)`` int64 words and every output a payload of exactly its shape; on arenas filled with 0x00
and with 0xFF, both results equal to the scalar restatement bit for bit; no guard band written; landmarks and uv come back bit for bit."""
import numpy as np
import pytest

from tests import guarded as G
from tests import pnp_p3p_ref as Q
from tests import pnp_ref as R

pytestmark = pytest.mark.gpu

HYPOTHESES, REFINE = 512, 4
ALL = R.OUTPUTS + R.HYPOTHESES


def _run(ftk, name, fill):
    import torch
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    X, uv, status = Q.case(name)
    n = len(X)
    specs = [("landmarks", "float32", (n, 3), 0), ("uv", "float32", (n, 2), 0), ("status", "uint8", (n,), 0),
             ("workspace", "int64", (-(-N.pnp_ransac_workspace_bytes(n, HYPOTHESES, REFINE) // 8),), 0), ("pose", "float32", (7,), 0),
             ("n_inliers", "int32", (1,), 0), ("best", "int32", (1,), 0), ("valid", "int32", (1,), 0), ("counts", "int32", (HYPOTHESES,), 0),
             ("models", "float32", (HYPOTHESES, 12), 0)]
    arena = G.Arena(specs, "cuda", fill=fill)
    inputs = dict(landmarks=X, uv=uv, status=status)
    for key, array in inputs.items():
        arena.put(key, array)
    D.pnp_ransac_sampled_device(ftk.default_context(), arena["landmarks"], arena["uv"], arena["status"], R.K, 1.0, HYPOTHESES, REFINE, 0, "p3p",
                                arena["workspace"], arena["pose"], arena["n_inliers"], arena["best"], arena["valid"], arena["counts"], arena["models"])
    torch.cuda.synchronize()
    host = arena.check()
    for key in ("landmarks", "uv"):
        assert arena.payload_bytes(key, host).tobytes() == np.ascontiguousarray(inputs[key]).tobytes(), f"the call changed its input {key}"
    r = R.Result()
    for key in ALL:
        setattr(r, key, arena[key].cpu().numpy())
    return r


@pytest.mark.parametrize("name", ["n3", "n4", "n64_half", "n256", "n257", "n1025", "hostile"])
def test_the_sampled_entry_in_its_declared_bytes(ftk, name):
    X, uv, status = Q.case(name)
    want = Q.solve(X, uv, status)
    for fill in (G.ZEROS, G.ONES):
        assert R.same_results(_run(ftk, name, fill), want, ALL) == [], (name, hex(fill))
