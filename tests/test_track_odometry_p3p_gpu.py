"""``TrackOdometry(pnp_sample="p3p")`` over a short sequence (64 slots, 8 frames) against the composition of the restatements with
tests/pnp_p3p_ref.py in ``PnpRansac``'s place, bit for bit after every frame.  tests/track_odometry_ref.py's
``Odometry`` calls tests/pnp_ref.py by name, so the composition with the other sampler is written here: its ``update`` with that one call
replaced."""
import numpy as np
import pytest

from tests import pnp_p3p_ref as Q
from tests import track_odometry_ref as O

pytestmark = pytest.mark.gpu

TENSORS = O.STATE + ("pnp_status", "anchor_status")
SLOTS, FRAMES, MIN_LANDMARKS = 64, 8, 12


class OdometryP3p(O.Odometry):
    """``O.Odometry`` whose steady state solves with the "p3p" restatement; the bootstrap is the parent's."""

    def update(self, ids, points, image_size=O.IMAGE):
        if not self.initialised:
            return super().update(ids, points, image_size)
        ids, points = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(points, np.float32)
        t, seed = self.table, (self.seed + self.frame) & 0xFFFFFFFF
        O.begin(t, ids, self.variant)
        fit = Q.solve(t.landmarks, points, t.pnp_status, self.K, self.hypotheses, self.threshold, self.refine_iterations, seed)
        t.pnp_status[:] = fit.status
        self._end(ids, points, O.STEADY, fit.pose, fit.valid)
        self.frame += 1
        return self


def _state(odo):
    t = O.Table(0)
    for name in TENSORS:
        setattr(t, name, getattr(odo, name).cpu().numpy())
    return t


def test_update_with_the_p3p_sampler_equals_the_composed_restatements_after_every_frame(ftk):
    import torch
    ids, points, _, _ = O.sequence(0.3, frames=FRAMES, n=SLOTS)
    odo = ftk.TrackOdometry(O.K, seed=5, min_landmarks=MIN_LANDMARKS, pnp_sample="p3p")
    want, other = OdometryP3p(seed=5, min_landmarks=MIN_LANDMARKS), O.Odometry(seed=5, min_landmarks=MIN_LANDMARKS)
    steady = 0
    for f in range(FRAMES):
        steady += want.initialised
        want.update(ids[f], points[f])
        other.update(ids[f], points[f])
        odo.update(torch.from_numpy(ids[f].copy()).cuda(), torch.from_numpy(points[f].copy()).cuda(), O.IMAGE)
        torch.cuda.synchronize()
        assert O.same_tables(want.table, _state(odo), TENSORS) == [], f
        assert (odo.initialised, odo.frame) == (want.initialised, want.frame)
        assert int(odo.valid[0]) == want.table.counters[O.VALID] and int(odo.n_landmarks[0]) == want.table.counters[O.N_LANDMARKS]
    assert steady >= 3 and want.table.counters[O.VALID] == 1 and want.table.counters[O.N_LANDMARKS] >= MIN_LANDMARKS
    assert O.same_tables(want.table, other.table, ("pose",)) == ["pose"]  # the sampler is in the result: "dlt6" ends on other bits
