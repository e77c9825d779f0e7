"""Raft(correlation="on_demand") on the device: its predictions are bit-identical to the scalar composition of the existing
encoder, update-block and upsampling restatements with the on-demand correlation restatement in place of the all-pairs one; their distance
to the float64 composition of the whole model (tests/test_raft_encoder_cpu.py's) is at most twice the all-pairs mode's on the same inputs;
and the default mode still gives what it gave: the restatement of the parent commit bit for bit, the recorded fixture within its bound.
Two inputs: the committed fixture tests/golden/raft/raft_model_small.npz (one correlation level, as every RAFT case of the suite: there the
two modes are one computation) and a 64 x 64 pair whose 8 x 8 feature maps carry three levels, where they are not.

Measured on an MI355X (printed by the tests, -s shows them): see DESIGN.md 5.16."""
import functools

import numpy as np
import pytest

from tests import flow_upsample_ref, raft_conv_ref
from tests import raft_corr_ondemand_ref as O
from tests import raft_encoder_ref as E
from tests.test_raft_encoder_cpu import GOLDEN, RAFT_BOUND, make_image, make_raft_state, max_abs, torch_raft

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# hidden, feature, context, levels, radius, corr_hidden, corr_out, flow_hidden, flow_out, motion_out, mask_hidden; B, H, W, iterations
THREE_LEVEL_CASE = (8, 12, 4, 3, 1, 8, 6, 8, 4, 10, 8, 1, 64, 64, 2)
ALLOWED_FACTOR = 2.0  # tests/test_raft_corr_ondemand_cpu.py's argument, carried through the iterations


def raft_on_demand_restated(ref_image, cur_image, state, levels, radius, iterations):
    """tests/raft_encoder_ref.py::raft with the on-demand correlation restatement in place of the pyramid."""
    ref_image, cur_image = E._f32(ref_image), E._f32(cur_image)
    B = ref_image.shape[0]
    features = E.feature_encoder(np.concatenate([ref_image, cur_image], 0), state, "feature_encoder.", True)
    block = raft_conv_ref.weights_of(state, "update_block.")
    net_channels = block["flow_head.conv1.weight"].shape[1]
    total = E._f32(state["context_encoder.net.conv_out.0.weight"]).shape[0]
    inp, net = E.context_encoder(ref_image, state, "context_encoder.", total - net_channels, True)
    h, w = features.shape[2:]
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    ref = np.ascontiguousarray(np.broadcast_to(np.stack([xs, ys])[None], (B, 2, h, w)))
    cur = ref
    predictions = []
    for _ in range(iterations):
        correlation = O.lookup(features[:B], features[B:], levels, cur, radius)
        flow = cur - ref
        net, mask, delta = raft_conv_ref.update_block(net, inp, correlation, flow, block)[:3]
        cur = cur + delta
        predictions.append(flow_upsample_ref.upsample(cur - ref, mask))
    return predictions


@functools.lru_cache(maxsize=None)
def case(name):
    """(state, ref_image, cur_image, levels, radius, iterations, recorded predictions or None) as numpy."""
    if name == "fixture":
        z = np.load(GOLDEN)
        state = {k[len("state/"):]: z[k] for k in z.files if k.startswith("state/")}
        sizes = [int(e) for e in z["sizes"]]
        return state, z["ref_image"], z["cur_image"], sizes[4], sizes[5], sizes[12], [z["prediction_0"], z["prediction_1"]]
    c = THREE_LEVEL_CASE
    state = make_raft_state(c, 1)
    B, H, W, iterations = c[11:]
    return ({k: v.numpy() for k, v in state.items()}, make_image(B, 1, H, W, 1).numpy(), make_image(B, 1, H, W, 71).numpy(), c[3], c[4], iterations, None)


@functools.lru_cache(maxsize=None)
def float64_predictions(name):
    state, ref_image, cur_image, levels, radius, iterations, _ = case(name)
    tensors = {k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}
    return [p.numpy() for p in torch_raft(tensors, torch.from_numpy(ref_image), torch.from_numpy(cur_image), levels, radius, iterations)]


@functools.lru_cache(maxsize=None)
def device_predictions(ftk, name, mode):
    state, ref_image, cur_image, levels, radius, iterations, _ = case(name)
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")  # noqa: E731
    kwargs = {} if mode is None else {"correlation": mode}
    model = ftk.Raft.from_state_dict({k: on(v) for k, v in state.items()}, levels, radius, max_iterations=iterations, **kwargs)
    assert model.correlation == (mode or "all_pairs")
    return [p.cpu().numpy() for p in model(on(ref_image), on(cur_image))]


@pytest.mark.parametrize("name", ["fixture", "three levels"])
def test_on_demand_bit_identical_to_the_scalar_composition(ftk, name):
    state, ref_image, cur_image, levels, radius, iterations, _ = case(name)
    want = raft_on_demand_restated(ref_image, cur_image, state, levels, radius, iterations)
    got = device_predictions(ftk, name, "on_demand")
    assert len(got) == len(want) == iterations
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and E.same(g, w), f"prediction {i} differs at {np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:5].tolist()}"


@pytest.mark.parametrize("name", ["fixture", "three levels"])
def test_distance_between_the_modes_against_float64(ftk, name):
    ref64 = float64_predictions(name)
    all_pairs = max_abs(device_predictions(ftk, name, "all_pairs"), ref64)
    on_demand = max_abs(device_predictions(ftk, name, "on_demand"), ref64)
    between = max_abs(device_predictions(ftk, name, "all_pairs"), device_predictions(ftk, name, "on_demand"))
    print(f"Raft {name}: all_pairs vs float64 {all_pairs:.3g}, on_demand vs float64 {on_demand:.3g} ({on_demand / all_pairs:.2f} x, allowed "
          f"{ALLOWED_FACTOR} x); between the modes {between:.3g}")
    assert all_pairs > 0
    assert on_demand <= ALLOWED_FACTOR * all_pairs
    if case(name)[3] == 1:
        assert between == 0  # one level: level 0 is the same chain in both modes


@pytest.mark.parametrize("name", ["fixture", "three levels"])
def test_default_mode_is_unchanged(ftk, name):
    state, ref_image, cur_image, levels, radius, iterations, recorded = case(name)
    default = device_predictions(ftk, name, None)
    want = E.raft(ref_image, cur_image, state, levels, radius, iterations)  # the all-pairs composition, as on the parent commit
    for i, (g, w) in enumerate(zip(default, want)):
        assert E.same(g, w), f"prediction {i}"
    for g, e in zip(default, device_predictions(ftk, name, "all_pairs")):
        assert E.same(g, e)  # the keyword's default is "all_pairs"
    if recorded is not None:
        print(f"default mode against the reference model's recorded float32 predictions: {max_abs(default, recorded):.3g} (bound {RAFT_BOUND:.3g})")
        assert max_abs(default, recorded) <= RAFT_BOUND
