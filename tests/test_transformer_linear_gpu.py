"""``linear_device`` alone (ftk_linear_device, LightGlue's input_proj) against the scalar restatement's ``linear``, bit for
bit: at the row edges of a wave and of a workgroup, the column edges of an MFMA tile and of a workgroup's tile, in_dim 1, odd and at the
limit (transformer_ref.LINEAR_CASES), and on NaN, inf, -0 and subnormals.  Every case runs both bodies of linear_kernel: with ``x`` and
``weight`` 16-byte aligned (the vector body where in_dim % 4 == 0) and with both one float into their payloads (the scalar body
whatever in_dim is).  Every tensor is a payload of guarded memory (tests/guarded.py): a store past a row or a column edge of ``out`` is
named, and the inputs come back bit for bit."""
import functools

import numpy as np
import pytest

from tests import guarded as G
from tests import transformer_ref as R

pytestmark = pytest.mark.gpu

BODIES = {"aligned": 0, "one_float_in": 1}


@functools.lru_cache(maxsize=None)
def _want(case, hostile):
    return R.linear(*(R.hostile_linear_case(*case) if hostile else R.linear_case(*case)))


def _run(ftk, case, shift, hostile, fill):
    import torch
    from feature_tracker_amd import device as D
    rows, ins, outs = case
    x, w, bias = R.hostile_linear_case(*case) if hostile else R.linear_case(*case)
    arena = G.Arena([("x", "float32", (rows * ins + shift,), 0), ("weight", "float32", (outs * ins + shift,), 0), ("bias", "float32", (outs,), 0),
                     ("out", "float32", (rows, outs), 0)], "cuda", fill=fill)
    given = dict(x=np.concatenate([np.full(shift, 7.0, np.float32), x.ravel()]), weight=np.concatenate([np.full(shift, 7.0, np.float32), w.ravel()]), bias=bias)
    for name, array in given.items():
        arena.put(name, array)
    d_x, d_w = arena["x"][shift:].view(rows, ins), arena["weight"][shift:].view(outs, ins)
    assert d_x.is_contiguous() and d_w.is_contiguous() and d_x.data_ptr() % 16 == 4 * shift and d_w.data_ptr() % 16 == 4 * shift
    D.linear_device(ftk.default_context(), d_x, d_w, arena["bias"], arena["out"])
    torch.cuda.synchronize()
    host = arena.check()
    for name, array in given.items():
        assert arena.payload_bytes(name, host).tobytes() == array.tobytes(), f"the call changed its input {name}"
    return arena["out"].cpu().numpy()


@pytest.mark.parametrize("body", sorted(BODIES))
@pytest.mark.parametrize("case", R.LINEAR_CASES, ids=lambda c: f"{c[0]}x{c[1]}to{c[2]}")
def test_linear_is_the_restatement_bit_for_bit(ftk, case, body):
    want = _want(case, False)
    assert np.isfinite(want).all()
    for fill in (G.ZEROS, G.ONES):
        assert R.same(_run(ftk, case, BODIES[body], False, fill), want), (case, body, hex(fill))


@pytest.mark.parametrize("body", sorted(BODIES))
@pytest.mark.parametrize("case", R.LINEAR_HOSTILE, ids=lambda c: f"{c[0]}x{c[1]}to{c[2]}")
def test_linear_with_hostile_inputs(ftk, case, body):
    """NaN, +-inf, -0 and subnormals through x, weight and bias, and a row of x that is all +0 against biases of -0: the sign of a zero
    result is where the k-step that pads an odd in_dim (5, scalar body) would show if it added anything.  The vector body runs at
    (8, aligned), the scalar body everywhere else."""
    want = _want(case, True)
    assert np.isnan(want).any() and np.isfinite(want).any() and ((want == 0) & np.signbit(want)).any()
    assert want[2, 1] == 0 and np.signbit(want[2, 1]) and want[2, 4] == 0 and not np.signbit(want[2, 4])
    for fill in (G.ZEROS, G.ONES):
        assert R.same(_run(ftk, case, BODIES[body], True, fill), want), (case, body, hex(fill))
