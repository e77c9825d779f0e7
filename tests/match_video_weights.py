"""Seeded random narrow networks for the tests of ``MatchVideoTracker``: TEST INFRASTRUCTURE.  The state dicts are the
other restatements' (tests/lightglue_adaptive_ref.py, tests/superpoint_ref.py), as torch tensors on the device asked for."""
import torch

from tests import lightglue_adaptive_ref as LA
from tests import superpoint_ref as SP


def lightglue_state(d=32, heads=2, layers=2, seed=0, device=None):
    """Upstream's names with ``token_confidence.{i}`` and ``log_assignment.{i}`` of every layer, so the same dict serves ``match`` and
    ``match_adaptive``."""
    sd = LA.state_dict(d, heads, seed + 500, n_layers=layers)
    return {k: torch.from_numpy(v.copy()).to(device or "cpu") for k, v in sd.items()}


def superpoint_state(d=32, seed=0, device=None):
    """A narrow SuperPoint: trunk widths 8, 8, 16, 16, heads of 32 hidden channels, ``d`` descriptor channels."""
    return {k: v.to(device or "cpu") for k, v in SP.make_state((8, 8, 16, 16, 32, d), seed).items()}
