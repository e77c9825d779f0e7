"""The landmark table's two entries and ``TrackOdometry`` on the device against the restatements (tests/landmark_table_ref.c,
tests/track_odometry_ref.py), bit for bit: every state tensor and counter at the sizes that cross the 256-slot workgroup
(five workgroups with one slot in the last; 65 536 slots), on tables in which every branch occurs, in both modes and with an invalid
pose; ``update`` over 12 frames of the sequence after every frame, one run with a frame whose landmark pixels are lost (not finite: PnP invalid) and one with
them redrawn (finite: the known limit, pinned); a
steady-state ``update`` replayed from a captured graph; both entries on guarded memory; ``KltVideoTracker(odometry=...)`` against the
tracker followed by ``update`` by hand."""
import numpy as np
import pytest

from tests import epipolar_ref as E
from tests import guarded as G
from tests import klt_video_cases as KV
from tests import track_odometry_ref as O

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1025, 65536)
TENSORS = O.STATE + ("pnp_status", "anchor_status")


class _Device:
    """A restatement table's tensors on the device."""

    def __init__(self, table):
        import torch
        for name in TENSORS:
            setattr(self, name, torch.from_numpy(getattr(table, name).copy()).cuda())

    def host(self):
        t = O.Table(0)
        for name in TENSORS:
            setattr(t, name, getattr(self, name).cpu().numpy())
        return t


def _begin(ftk, d, ids):
    from feature_tracker_amd import device as D
    D.landmark_table_begin_device(ftk.default_context(), ids, d.owner, d.landmarks, d.anchor_frame, d.pnp_status, d.anchor_status, d.counters)


def _end(ftk, d, ids, points, status, pose, valid, model, frame, mode):
    import torch
    from feature_tracker_amd import device as D
    up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()  # noqa: E731
    D.landmark_table_end_device(ftk.default_context(), ids, points, up(status, np.uint8), up(pose, np.float32), up(valid, np.int32), up(model, np.int32), frame, mode,
                                O.K, 1.0, O.cos2(1.0), d.landmarks, d.anchor_uv, d.anchor_pose, d.anchor_frame, d.counters, d.pose)


@pytest.mark.parametrize("n", SIZES)
def test_both_entries_bit_for_bit_on_every_branch(ftk, n):
    import torch
    table, ids, points, status, pose = O.branch_table(n)
    d_ids, d_points = torch.from_numpy(ids).cuda(), torch.from_numpy(points).cuda()
    start = table.copy()
    d = _Device(table)
    O.begin(table, ids)
    _begin(ftk, d, d_ids)
    torch.cuda.synchronize()
    assert O.same_tables(table, d.host(), TENSORS) == [], ("begin", n)
    after_begin = table.copy()
    for mode, valid, model in ((O.STEADY, [1], None), (O.BOOTSTRAP, [1], [0]), (O.STEADY, [-1], None), (O.BOOTSTRAP, [1], [1])):
        want, d = after_begin.copy(), _Device(after_begin)
        want.counters[O.LOST] = 2
        d.counters[O.LOST] = 2
        O.end(want, ids, points, status if mode == O.STEADY else None, pose, valid, model, 9, mode)
        _end(ftk, d, d_ids, d_points, status if mode == O.STEADY else None, pose, valid, model, 9, mode)
        torch.cuda.synchronize()
        assert O.same_tables(want, d.host(), TENSORS) == [], (mode, valid, model, n)
        if valid == [1] and model != [1] and n >= 13:
            assert want.counters[O.N_NEW] > 0 and O.same_tables(want, after_begin, ("landmarks", "counters")) != []
    assert E.same(d_ids.cpu().numpy(), ids) and E.same(d_points.cpu().numpy(), points) and O.same_tables(start, after_begin, ("anchor_uv",)) == []


def _state(odo):
    t = O.Table(0)
    for name in TENSORS:
        setattr(t, name, getattr(odo, name).cpu().numpy())
    return t


@pytest.mark.parametrize("how", [None, "lost", "scrambled"])
def test_update_over_twelve_frames_equals_the_restatement_after_every_frame(ftk, how):
    import torch
    ids, points, _, _ = O.sequence(0.3)
    odo, want = ftk.TrackOdometry(O.K, seed=5), O.Odometry(seed=5)
    for f in range(12):
        uv = points[f].copy()
        if f == 8 and how is not None:
            holders = (want.table.landmarks != 0).any(1)
            if how == "lost":  # every pixel of a landmark holder not finite: PnP has no participant and finds no pose
                uv[holders] = np.float32(np.nan)
            else:  # redrawn in the image: PnpRansac calls six finite points that form a model valid (the known limit)
                uv[holders] = np.random.default_rng(3).uniform([5, 5], [635, 475], (int(holders.sum()), 2)).astype(np.float32)
        want.update(ids[f], uv)
        odo.update(torch.from_numpy(ids[f].copy()).cuda(), torch.from_numpy(uv).cuda(), O.IMAGE)
        torch.cuda.synchronize()
        assert O.same_tables(want.table, _state(odo), TENSORS) == [], f
        assert (odo.initialised, odo.frame) == (want.initialised, want.frame)
        assert int(odo.valid[0]) == want.table.counters[O.VALID] and int(odo.n_landmarks[0]) == want.table.counters[O.N_LANDMARKS]
        if f == 8 and how == "lost":
            assert want.initialised and want.table.counters[O.VALID] == -1 and want.table.counters[O.LOST] == 1
        if f == 8 and how == "scrambled":  # accepted, and the map is gone: the limit as it stands
            assert want.table.counters[O.VALID] == 1 and want.table.counters[O.N_LANDMARKS] < 6
    if how == "scrambled":
        assert want.table.counters[O.VALID] == -1 and want.table.counters[O.LOST] == 3
    else:
        assert want.initialised and want.table.counters[O.VALID] == 1 and want.table.counters[O.N_LANDMARKS] >= 30


def test_a_steady_update_replayed_from_a_captured_graph_equals_the_eager_call(ftk):
    import torch
    ids, points, _, _ = O.sequence(0.3)
    odo = ftk.TrackOdometry(O.K, seed=5)
    d_ids, d_points = torch.from_numpy(ids[0].copy()).cuda(), torch.from_numpy(points[0].copy()).cuda()
    for f in range(7):
        d_ids.copy_(torch.from_numpy(ids[f].copy()))
        d_points.copy_(torch.from_numpy(points[f].copy()))
        odo.update(d_ids, d_points, O.IMAGE)
    assert odo.initialised and odo.frame == 7
    d_ids.copy_(torch.from_numpy(ids[7].copy()))
    d_points.copy_(torch.from_numpy(points[7].copy()))
    saved = {name: getattr(odo, name).clone() for name in TENSORS}
    odo.update(d_ids, d_points, O.IMAGE)  # the eager call of the size: the workspace is made here, outside the capture
    torch.cuda.synchronize()
    eager = _state(odo)
    for name in TENSORS:
        getattr(odo, name).copy_(saved[name])
    odo.frame = 7
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        odo.update(d_ids, d_points, O.IMAGE)
    for name in TENSORS:  # (the capture ran nothing; the state is put back all the same)
        getattr(odo, name).copy_(saved[name])
    graph.replay()
    torch.cuda.synchronize()
    assert O.same_tables(eager, _state(odo), TENSORS) == [] and int(odo.valid[0]) == 1 and eager.counters[O.N_LANDMARKS] >= 30


@pytest.mark.parametrize("n", [1, 257, 1025])
def test_both_entries_in_their_declared_bytes(ftk, n):
    import torch
    from feature_tracker_amd import device as D
    table, ids, points, status, pose = O.branch_table(n)
    want = table.copy()
    O.begin(want, ids)
    after_begin = want.copy()
    O.end(want, ids, points, status, pose, [1], None, 9, O.STEADY)
    specs = [("ids", "int64", (n,), 0), ("points", "float32", (n, 2), 0), ("status_in", "uint8", (n,), 0), ("pose_in", "float32", (7,), 0), ("valid_in", "int32", (1,), 0),
             ("owner", "int64", (n,), 0), ("landmarks", "float32", (n, 3), 0), ("anchor_uv", "float32", (n, 2), 0), ("anchor_pose", "float32", (n, 7), 0),
             ("anchor_frame", "int32", (n,), 0), ("pnp_status", "uint8", (n,), 0), ("anchor_status", "uint8", (n,), 0), ("counters", "int32", (O.COUNTERS,), 0),
             ("pose", "float32", (7,), 0)]
    for fill in (G.ZEROS, G.ONES):
        arena = G.Arena(specs, "cuda", fill=fill)
        inputs = dict(ids=ids, points=points, status_in=status, pose_in=pose, valid_in=np.array([1], np.int32), owner=table.owner, landmarks=table.landmarks,
                      anchor_uv=table.anchor_uv, anchor_pose=table.anchor_pose, anchor_frame=table.anchor_frame, counters=table.counters, pose=table.pose)
        for key, array in inputs.items():
            arena.put(key, array)
        ctx = ftk.default_context()
        D.landmark_table_begin_device(ctx, arena["ids"], arena["owner"], arena["landmarks"], arena["anchor_frame"], arena["pnp_status"], arena["anchor_status"],
                                      arena["counters"])
        torch.cuda.synchronize()
        arena.check()
        got = O.Table(0)
        for name in TENSORS:
            setattr(got, name, arena[name].cpu().numpy())
        assert O.same_tables(after_begin, got, TENSORS) == [], ("begin", n, hex(fill))
        D.landmark_table_end_device(ctx, arena["ids"], arena["points"], arena["status_in"], arena["pose_in"], arena["valid_in"], None, 9, O.STEADY, O.K, 1.0,
                                    O.cos2(1.0), arena["landmarks"], arena["anchor_uv"], arena["anchor_pose"], arena["anchor_frame"], arena["counters"], arena["pose"])
        torch.cuda.synchronize()
        host = arena.check()
        for key in ("ids", "points", "status_in", "pose_in", "valid_in"):
            assert arena.payload_bytes(key, host).tobytes() == np.ascontiguousarray(inputs[key]).tobytes(), f"the call changed its input {key}"
        for name in TENSORS:
            setattr(got, name, arena[name].cpu().numpy())
        assert O.same_tables(want, got, TENSORS) == [], ("end", n, hex(fill))


def test_the_tracker_with_odometry_equals_the_tracker_then_update_by_hand(ftk):
    """On the frames of tests/klt_video_cases.py.  They show one plane that moves in the image: "auto" chooses the homography on every pair,
    so the bootstrap does not complete there; what is held is that the wiring is the hand composition, bit for bit."""
    import torch
    from feature_tracker_amd import device as D

    def run(wired):
        ctx = D.context_on_stream(torch.cuda.Stream())
        flow = ftk.OpticalFlowBasicKlt()
        flow.options().kMethod = "fast"
        flow.options().kMaxTrackPointsNumber = 500
        odo = ftk.TrackOdometry((128.0, 128.0, 79.5, 59.5), min_landmarks=8, seed=2, ctx=ctx)
        tracker = ftk.KltVideoTracker(flow, 64, levels=KV.LEVELS, min_distance=KV.MIN_DISTANCE, min_response=KV.MIN_RESPONSE, ctx=ctx, odometry=odo if wired else None)
        states = []
        for image in KV.frames((3.3, -2.1), 0.0):
            tracker.track(image)
            if not wired:
                odo.update(tracker.ids, tracker.points, (KV.HEIGHT, KV.WIDTH))
            torch.cuda.synchronize()
            states.append((_state(odo), tracker.ids.cpu().numpy(), tracker.points.cpu().numpy(), odo.initialised, odo.frame))
        return states

    for (a, ids_a, uv_a, init_a, frame_a), (b, ids_b, uv_b, init_b, frame_b) in zip(run(True), run(False)):
        assert O.same_tables(a, b, TENSORS) == [] and E.same(ids_a, ids_b) and E.same(uv_a, uv_b) and (init_a, frame_a) == (init_b, frame_b)
    assert frame_a == KV.FRAMES and not init_a and (a.anchor_frame[ids_a >= 0] >= 0).sum() >= 8  # (a track born during the bootstrap has no anchor yet)


def test_the_refusals_of_the_library(ftk):
    import torch
    from feature_tracker_amd import _native as N
    ctx = ftk.default_context()
    i64, f32 = torch.zeros(16, dtype=torch.int64, device="cuda"), torch.zeros(16 * 7, device="cuda")
    i32, u8 = torch.zeros(16, dtype=torch.int32, device="cuda"), torch.zeros(16, dtype=torch.uint8, device="cuda")
    valid = torch.zeros(1, dtype=torch.int32, device="cuda")  # an invalid pose: the one call that launches changes nothing but lost
    p = lambda t: t.data_ptr()  # noqa: E731
    begin = lambda n=16: N.lib().ftk_landmark_table_begin_device(ctx.handle, None, p(i64), n, p(i64), p(f32), p(i32), p(u8), p(u8), p(i32))  # noqa: E731
    end = lambda n=16, frame=0, mode=0, fx=500.0, threshold=1.0, c2=0.5, status=True: N.lib().ftk_landmark_table_end_device(  # noqa: E731
        ctx.handle, None, p(i64), p(f32), n, p(u8) if status else None, p(f32), p(valid), None, frame, mode, fx, 500.0, 320.0, 240.0, threshold, c2, p(f32), p(f32), p(f32),
        p(i32), p(i32), p(f32))
    nan = float("nan")
    assert begin(0) == -1 and begin(N.FTK_TRACK_TABLE_MAX_SLOTS + 1) == -4 and end(0) == -1 and end(N.FTK_TRACK_TABLE_MAX_SLOTS + 1) == -4
    assert end(frame=-1) == -1 and end(mode=2) == -1 and end(fx=0.0) == -1 and end(fx=nan) == -1 and end(threshold=-1.0) == -1 and end(threshold=2.0e19) == -1
    assert end(c2=-0.1) == -1 and end(c2=1.5) == -1 and end(c2=nan) == -1 and end(status=False) == -1 and end(status=False, mode=1) == 0
    torch.cuda.synchronize()
