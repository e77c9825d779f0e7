"""``transformer_layer_device`` held to the sizes it declares, as tests/test_workspace_contract_gpu.py holds the other
entries: called directly on guarded memory (tests/guarded.py), the workspace exactly ``ceil(ftk_transformer_layer_workspace_bytes / 8)``
int64 words and every output a payload of exactly its shape; twice on fresh arenas, all payloads 0x00 and all 0xFF, both results equal to
the scalar restatement bit for bit; no guard band written; the inputs, guarded payloads too, come back bit for bit."""
import numpy as np
import pytest

from tests import guarded as G
from tests import transformer_ref as R

pytestmark = pytest.mark.gpu


def _run(ftk, shape, counts, fill):
    import torch
    from feature_tracker_amd import _native as N
    from feature_tracker_amd import device as D
    m, n, d, h, _ = shape
    a, b, e0, e1, sd = R.layer_case(shape)
    layer = ftk.TransformerLayer.from_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, "transformers.0.", h)
    packed = next(iter(layer._packed.values())).numpy()
    assert packed.size == N.transformer_layer_weight_offsets(d)[2]
    inputs = dict(desc0=a, desc1=b, enc0=e0, enc1=e1, weights=packed)
    specs = [("desc0", "float32", (m, d), 0), ("desc1", "float32", (n, d), 0), ("enc0", "float32", (2, m, d // h), 0), ("enc1", "float32", (2, n, d // h), 0),
             ("weights", "float32", (packed.size,), 0)]
    if counts is not None:
        specs += [("count0", "int32", (1,), 0), ("count1", "int32", (1,), 0)]
        inputs.update(count0=np.array([counts[0]], np.int32), count1=np.array([counts[1]], np.int32))
    specs += [("workspace", "int64", (-(-N.transformer_layer_workspace_bytes(m, n, d, h) // 8),), 0), ("out0", "float32", (m, d), 0), ("out1", "float32", (n, d), 0)]
    arena = G.Arena(specs, "cuda", fill=fill)
    for name, array in inputs.items():
        arena.put(name, array)
    D.transformer_layer_device(ftk.default_context(), arena["desc0"], arena["desc1"], h, arena["enc0"], arena["enc1"], arena["weights"],
                               arena["count0"] if counts is not None else None, arena["count1"] if counts is not None else None, arena["workspace"],
                               arena["out0"], arena["out1"])
    torch.cuda.synchronize()
    host = arena.check()
    for name, array in inputs.items():
        assert arena.payload_bytes(name, host).tobytes() == np.ascontiguousarray(array).tobytes(), f"the call changed its input {name}"
    return arena["out0"].cpu().numpy(), arena["out1"].cpu().numpy()


GUARDED_SHAPES = R.LAYER_SHAPES[:4] + R.LAYER_NARROW  # the latter: D % 4 != 0, the non-vector Linear and attention


@pytest.mark.parametrize("shape", GUARDED_SHAPES, ids=["x".join(str(v) for v in s[:4]) for s in GUARDED_SHAPES])
def test_the_layer_in_its_declared_bytes(ftk, shape):
    import ctypes as C
    from feature_tracker_amd import _native as N
    m, n, d, h, _ = shape
    declared = C.c_int64()
    assert N.lib().ftk_transformer_layer_workspace_bytes(m, n, d, h, C.byref(declared)) == 0
    assert declared.value == N.transformer_layer_workspace_bytes(m, n, d, h)
    a, b, e0, e1, sd = R.layer_case(shape)
    for counts in (None, ((2 * m + 2) // 3, (3 * n + 3) // 4)):
        want = R.layer(a, b, h, e0, e1, sd) if counts is None else R.layer(a, b, h, e0, e1, sd, count0=counts[0], count1=counts[1])
        for fill in (G.ZEROS, G.ONES):
            got = _run(ftk, shape, counts, fill)
            assert R.same(got[0], want[0]) and R.same(got[1], want[1]), (shape, counts, hex(fill))
