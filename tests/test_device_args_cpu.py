"""The argument checks of feature_tracker_amd/device.py, without a device.

The torch entries hand ``data_ptr()`` and a few counts to a C ABI that cannot see dtype, shape or strides, so what the caller meant and
what the kernel reads agree only if the Python layer holds every tensor to the ABI's contract first.  Two things are pinned here:

* ``_tensor_complaint``, the pure metadata half of the check, over a table of CPU tensors: every dtype, rank, shape position and stride
  pattern it must refuse, and the views it must keep accepting;
* a walk over EVERY public entry of the module with duck-typed tensors and a recording stand-in for the native library: no entry may
  reach ``data_ptr()`` of an argument that did not pass through ``_check``, and an entry this file does not know fails the walk — the
  guard that keeps the next entry from being added unchecked.  (The GPU half, refusals with the native entry stubbed and bit parity of
  what stays legal, is tests/test_device_args_gpu.py.)"""
import inspect

import pytest
import torch

import feature_tracker_amd as F
from feature_tracker_amd import _native as N
from feature_tracker_amd import device as D
from tests.args_walk import Fake, FakeDevice, Walk

F32, U8, I32, WORDS = ("float32",), ("uint8",), ("int32",), ("int32", "uint32")


def _t(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


# (what, tensor, allowed dtypes, expected shape, min_numel, substring of the complaint or None where the tensor is legal)
TABLE = [
    # dtype
    ("float32 pairs", _t(8, 2), F32, (None, 2), None, None),
    ("float64 pairs (torch.from_numpy of a default numpy array)", _t(8, 2, dtype=torch.float64), F32, (None, 2), None, "wrong dtype"),
    ("float16 pairs", _t(8, 2, dtype=torch.float16), F32, (None, 2), None, "wrong dtype"),
    ("int64 index_pairs (torch.full((n,), -1))", torch.full((8,), -1), I32, (8,), None, "wrong dtype"),
    ("bool status", _t(8, dtype=torch.bool), U8, (8,), None, "wrong dtype"),
    ("int32 status", _t(8, dtype=torch.int32), U8, (8,), None, "wrong dtype"),
    ("int8 status", _t(8, dtype=torch.int8), U8, (8,), None, "wrong dtype"),
    ("int64 iters", _t(8, dtype=torch.int64), ("int32", "uint32"), (8,), None, "wrong dtype"),
    ("int32 words", _t(8, 3, dtype=torch.int32), WORDS, (None, None), None, None),
    ("uint32 words", _t(8, 3, dtype=torch.uint32), WORDS, (None, None), None, None),
    ("uint8 words (unpacked bits)", _t(8, 96, dtype=torch.uint8), WORDS, (None, None), None, "wrong dtype"),
    ("int64 words", _t(8, 3, dtype=torch.int64), WORDS, (None, None), None, "wrong dtype"),
    # rank
    ("flat pairs", _t(16), F32, (None, 2), None, "1 dimensions instead of 2"),
    ("batched pairs", _t(1, 8, 2), F32, (None, 2), None, "3 dimensions instead of 2"),
    ("status as a column", _t(8, 1, dtype=torch.uint8), U8, (8,), None, "2 dimensions instead of 1"),
    ("0-d pose", torch.tensor(1.0), F32, (7,), None, "0 dimensions instead of 1"),
    # each shape position
    ("[n, 3] points as pairs", _t(8, 3), F32, (None, 2), None, "dimension 1 is 3, not 2"),
    ("one pair short", _t(7, 2), F32, (8, 2), None, "dimension 0 is 7, not 8"),
    ("one pair long", _t(9, 2), F32, (8, 2), None, "dimension 0 is 9, not 8"),
    ("one status short", _t(7, dtype=torch.uint8), U8, (8,), None, "dimension 0 is 7, not 8"),
    ("narrower partner", _t(9, 7, dtype=torch.int32), WORDS, (None, 8), None, "dimension 1 is 7, not 8"),
    ("pose of 6", _t(6), F32, (7,), None, "dimension 0 is 6, not 7"),
    ("[dim, n] descriptors against dim", _t(16, 8), F32, (None, 16), None, "dimension 1 is 8, not 16"),
    # flat buffers the ABI sizes itself
    ("shard of the exact size", _t(80, dtype=torch.uint8), U8, (None,), 80, None),
    ("shard with room", _t(96, dtype=torch.uint8), U8, (None,), 80, None),
    ("shard one byte short", _t(79, dtype=torch.uint8), U8, (None,), 80, "79 elements are too few"),
    # strides
    ("transposed [dim, n] descriptors", _t(16, 8).t(), F32, (None, 16), None, ".contiguous()"),
    ("column slice of [n, 3] points", _t(8, 3)[:, :2], F32, (None, 2), None, ".contiguous()"),
    ("every other row", _t(16, 2)[::2], F32, (8, 2), None, ".contiguous()"),
    ("every other status", _t(16, dtype=torch.uint8)[::2], U8, (8,), None, ".contiguous()"),
    ("expanded row (stride 0)", _t(1, 2).expand(8, 2), F32, (8, 2), None, ".contiguous()"),
    ("expanded scalar status", _t(1, dtype=torch.uint8).expand(8), U8, (8,), None, ".contiguous()"),
    ("reversed rows are a copy in torch: flip is dense", _t(8, 2).flip(0), F32, (8, 2), None, None),
    # views that stay legal
    ("row slice at an offset", _t(20, 2)[3:11], F32, (8, 2), None, None),
    ("row slice of words at an odd row", _t(20, 3, dtype=torch.int32)[1:9], WORDS, (None, 3), None, None),
    ("status at an odd offset", _t(20, dtype=torch.uint8)[3:11], U8, (8,), None, None),
    ("view of a flat buffer one float in", _t(17)[1:].view(8, 2), F32, (8, 2), None, None),
    ("[1, d] row", _t(1, 16), F32, (None, 16), None, None),
    ("[1, d] row of a transposed [d, 1] column (extent-1 strides are arbitrary)", _t(16, 1).t(), F32, (None, 16), None, None),
    ("[1, 2] pair cut out of [1, 3]", _t(1, 3)[:, :2], F32, (None, 2), None, None),
    ("[d, 1] column slice of [d, 3] is strided", _t(16, 3)[:, :1], F32, (16, 1), None, ".contiguous()"),
    # zero size
    ("no features", _t(0, 2), F32, (None, 2), None, None),
    ("no features, any strides", _t(0, 3)[:, :2], F32, (None, 2), None, None),
    ("no status", _t(4, dtype=torch.uint8)[:0], U8, (0,), None, None),
    ("no features but the wrong width", _t(0, 3), F32, (None, 2), None, "dimension 1 is 3, not 2"),
    ("no features but the wrong dtype", _t(0, 2, dtype=torch.float64), F32, (None, 2), None, "wrong dtype"),
    # not a tensor
    ("a numpy array", _t(8, 2).numpy(), F32, (None, 2), None, "must be a torch tensor"),
    ("None", None, F32, (None, 2), None, "must be a torch tensor"),
]


@pytest.mark.parametrize("what,t,dtypes,shape,min_numel,expect", TABLE, ids=[row[0] for row in TABLE])
def test_metadata_complaint(what, t, dtypes, shape, min_numel, expect):
    got = D._tensor_complaint("arg_x", t, dtypes, shape, min_numel)
    if expect is None:
        assert got is None, got
    else:
        assert got is not None, f"{what}: accepted"
        assert got.startswith("arg_x must be") and expect in got, got


def test_the_check_raises_the_complaint_and_refuses_host_tensors():
    """``_check`` = the metadata complaint, else the device complaint, as a ValueError that names the argument; a CPU tensor that is
    otherwise right is refused for where it lives, and nothing is converted or copied on the way."""
    good = _t(8, 2)
    with pytest.raises(ValueError, match=r"^ref_uv must be a CUDA tensor"):
        D._check("ref_uv", good, F32, (None, 2), None)
    with pytest.raises(ValueError, match=r"^ref_uv must be .*wrong dtype"):
        D._check("ref_uv", good.double(), F32, (None, 2), None)
    with pytest.raises(ValueError, match=r"pass ref_desc\.contiguous\(\)"):
        D._check("ref_desc", _t(16, 8).t(), F32, (None, 16), None)
    fake = Fake("x", "float32", (8, 2), set(), [], device=FakeDevice(1))
    assert D._device_complaint("x", fake, None) is None
    assert D._device_complaint("x", fake, 1) is None
    assert "must be on cuda:0" in D._device_complaint("x", fake, 0)


# ---- the walk (its duck-typed tensors and recording library: tests/args_walk.py) ----------------------------------------------------


def _direct_problem(w, k):
    return dict(ref=w.pyr, cur=w.pyr, K=[1.0, 1.0, 0.0, 0.0], p_c_in_ref=w.t(f"p_c_in_ref{k}", "float32", 8, 3), ref_uv=w.t(f"ref_uv{k}", "float32", 8, 2),
                cur_uv=w.t(f"cur_uv{k}", "float32", 8, 2), pose=w.t(f"pose{k}", "float32", 7), status=w.t(f"status{k}", "uint8", 8),
                iterations=w.t(f"iterations{k}", "int32", 1))


# entry -> (a call of it with every tensor argument present and right, the native entry point it must reach)
RECIPES = {
    "pyramid_from_tensors": (lambda w: D.pyramid_from_tensors([w.t("level0", "uint8", 12, 16), w.t("level1", "uint8", 6, 8)], w.ctx), "ftk_pyramid_wrap_device"),
    "DeviceKlt.bind": (lambda w: w.klt().bind(*w.klt_in(), *w.klt_out(), w.t("iters", "int32", 8))(), "ftk_klt_track_device"),
    "DeviceKlt.track": (lambda w: w.klt().track(*w.klt_in(), *w.klt_out(), w.t("iters", "int32", 8)), "ftk_klt_track_device"),
    "DeviceKlt.track_sharded": (lambda w: w.klt().track_sharded(w.comm, *w.klt_in(), *w.klt_out(), w.t("iters", "int32", 8)), "ftk_klt_track_sharded_device"),
    "DeviceKlt.bind_sharded": (lambda w: w.klt().bind_sharded(w.comm, *w.klt_in(), *w.klt_out())(), "ftk_klt_track_sharded_device"),
    "DeviceKlt.track_shard": (lambda w: w.klt().track_shard(1, 3, *w.klt_in(), w.t("packed_shard", "uint8", 32), w.t("iters", "int32", 8)),
                              "ftk_klt_track_shard_device"),
    "DeviceKlt.unpack_shards": (lambda w: w.klt().unpack_shards(w.t("gathered", "uint8", 96), 8, 3, *w.klt_out()), "ftk_klt_unpack_shards_device"),
    "hamming_match_sharded_device": (lambda w: D.hamming_match_sharded_device(w.ctx, w.comm, w.t("ref_words", "int32", 8, 3), w.t("cur_words", "uint32", 9, 3), 96, 20.0,
                                                                              w.t("index_pairs", "int32", 8), **w.nearby()), "ftk_hamming_match_sharded_device"),
    "hamming_match_device": (lambda w: D.hamming_match_device(w.ctx, w.t("ref_words", "int32", 8, 3), w.t("cur_words", "int32", 9, 3), 96, 20.0, w.t("index_pairs", "int32", 8),
                                                              workspace=w.t("workspace", "int64", 8), **w.nearby()), "ftk_hamming_match_device"),
    "cosine_match_device": (lambda w: D.cosine_match_device(w.ctx, w.t("ref_desc", "float32", 8, 16), w.t("cur_desc", "float32", 9, 16), 0.3, w.t("index_pairs", "int32", 8),
                                                            **w.nearby()), "ftk_cosine_match_device"),
    "brief_compute_device": (lambda w: D.brief_compute_device(w.ctx, w.pyr, w.t("uv", "float32", 8, 2), 96, 8, w.t("words_out", "int32", 8, 3)), "ftk_brief_compute_device"),
    "DeviceDirectBatch": (lambda w: D.DeviceDirectBatch(F.DirectMethodOptions(), [_direct_problem(w, 0), _direct_problem(w, 1)], w.ctx).track(),
                          "ftk_direct_track_batch_device"),
    "dense_flow_device": (lambda w: D.dense_flow_device(w.ctx, F.DenseOpticalFlowOptions(), w.pyr, w.pyr, w.t("flow_r", "float32", 12, 16), w.t("flow_c", "float32", 12, 16)),
                          "ftk_dense_flow_device"),
    "corr_pyramid_build_device": (lambda w: D.corr_pyramid_build_device(w.ctx, w.t("fmap0", "float32", 1, 4, 4, 6), w.t("fmap1", "float32", 1, 4, 4, 6), 1,
                                                                        w.t("volume", "float32", 576)), "ftk_corr_pyramid_build_device"),
    "corr_pyramid_lookup_device": (lambda w: D.corr_pyramid_lookup_device(w.ctx, w.t("volume", "float32", 576), 1, 1, w.t("coords", "float32", 1, 2, 4, 6),
                                                                          w.t("out", "float32", 1, 9, 4, 6)), "ftk_corr_pyramid_lookup_device"),
}
# entries that take no tensor: nothing of theirs can be misread
NO_TENSOR_ARGUMENT = {"context_on_stream", "upload_pyramid", "shard_bounds", "Comm", "Comm.unique_id", "Comm.close", "DeviceKlt", "DeviceDirectBatch.track"}
# entries that hold their tensors to torch's own types inline (isinstance(torch.Tensor), a strided score matrix): no duck-typed tensor
# passes them; their refusals are asserted in tests/test_nn_match_gpu.py
CHECKED_INLINE = {"nn_match_scores_device", "nn_match_list_device", "nn_fill_pixels_device"}


def _public_entries():
    names = set()
    for name, obj in vars(D).items():
        if name.startswith("_") or getattr(obj, "__module__", None) != D.__name__:
            continue
        if inspect.isfunction(obj):
            names.add(name)
        elif inspect.isclass(obj):
            names.add(name)
            for member, f in vars(obj).items():
                if not member.startswith("_") and (inspect.isfunction(f) or isinstance(f, (staticmethod, classmethod))):
                    names.add(f"{name}.{member}")
    return names


def test_every_public_entry_is_known_to_the_walk():
    """A new entry of device.py must be given a recipe below (or a reason why it needs none) before this passes."""
    known = set(RECIPES) | NO_TENSOR_ARGUMENT | CHECKED_INLINE
    assert _public_entries() == known, sorted(_public_entries() ^ known)


@pytest.mark.parametrize("entry", sorted(RECIPES))
def test_no_entry_takes_a_pointer_of_an_unchecked_argument(entry, monkeypatch):
    """With every argument right the entry reaches its native function, has taken ``data_ptr()`` of every tensor it was given, and of
    none before that tensor passed ``_check``."""
    call, native = RECIPES[entry]
    w = Walk(monkeypatch)
    call(w)
    assert w.unchecked_reads == [], f"{entry}: data_ptr() of {w.unchecked_reads} taken without a check"
    assert native in w.lib.calls, f"{entry}: the walk's call was refused before {native} ({w.lib.calls})"
    never_read = [f.name for f in w.made if f.reads == 0]
    assert never_read == [], f"{entry}: the walk passed {never_read} but the entry never used them; the recipe is out of date"


def test_the_walk_notices_an_unchecked_pointer(monkeypatch):
    """The guard itself: an entry written the old way (pointer first, no check) is reported."""
    w = Walk(monkeypatch)

    def old_style_entry(ctx, uv, status):
        D._check("uv", uv, F32, (None, 2), 0)
        return N.lib().ftk_something_device(ctx.handle, uv.data_ptr(), status.data_ptr(), uv.shape[0])

    old_style_entry(w.ctx, w.t("uv", "float32", 8, 2), w.t("status", "uint8", 8))
    assert w.unchecked_reads == ["status"] and w.lib.calls == ["ftk_something_device"]


@pytest.mark.parametrize("entry", sorted(set(RECIPES) - {"pyramid_from_tensors", "corr_pyramid_build_device", "corr_pyramid_lookup_device", "dense_flow_device"}))
def test_a_refused_argument_stops_the_entry_before_the_library(entry, monkeypatch):
    """Each tensor argument of each entry in turn made float64 / int64: ValueError, and the recording library saw no launch."""
    call, native = RECIPES[entry]
    probe = Walk(monkeypatch)
    call(probe)
    for k in range(len(probe.made)):
        w = Walk(monkeypatch, spoil=(k, "dtype", "float64"))
        with pytest.raises(ValueError, match=probe.made[k].name.rstrip("01")):
            call(w)
        assert [c for c in w.lib.calls if c.endswith("_device")] == [], (entry, probe.made[k].name, w.lib.calls)
        assert w.unchecked_reads == []
