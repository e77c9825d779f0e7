"""Device-resident entry points for callers that already hold their data in HBM (torch tensors).

PyTorch is plumbing here: it owns the device memory and the HIP stream; the computation is the
``ftk_*_device`` part of the C ABI (hand-written HIP kernels).  Used by bench.py, the smoke test
and the multi-GPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _native as N
from ._torch_call import stream_or_current
from .tracker import Context, ImagePyramid, OpticalFlowOptions


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("feature_tracker_amd.device needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch


_F32, _U8, _I32 = ("float32",), ("uint8",), ("int32",)
_WORDS = ("int32", "uint32")   # bit patterns: the kernels read uint32, torch callers usually hold int32
_COUNTS = ("int32", "uint32")  # the ABI writes uint32 iteration counts
_KEYS = ("int64", "uint64")


def _tensor_complaint(name, t, dtypes, shape, min_numel=None):
    """The dtype / rank / shape / stride half of an argument check: what is wrong with ``t`` as argument ``name``, or None.  A pure
    function of tensor metadata (dtype, shape, strides), so a CPU tensor answers like a CUDA one.  ``dtypes``: allowed torch dtype
    names; ``shape``: one entry per dimension, an extent or None for any; ``min_numel``: least element count (flat buffers the ABI
    sizes in bytes or words).  Dense row-major only: the C ABI sees a pointer and counts, never a stride."""
    if not hasattr(t, "data_ptr") or not hasattr(t, "stride"):
        return f"{name} must be a torch tensor (got {type(t).__name__})"
    want = "[" + ", ".join("*" if e is None else str(int(e)) for e in shape) + "]" + ("" if min_numel is None else f" with at least {int(min_numel)} elements")
    expected = f"{name} must be a contiguous {' or '.join(dtypes)} tensor of shape {want}"
    got_shape, got_stride = tuple(int(e) for e in t.shape), tuple(int(e) for e in t.stride())
    got = f"got {t.dtype} {list(got_shape)} with strides {list(got_stride)}"
    if str(t.dtype) not in tuple("torch." + d for d in dtypes):
        return f"{expected}: wrong dtype ({got}); there is no conversion here, the kernels read the bytes as they are"
    if len(got_shape) != len(shape):
        return f"{expected}: {len(got_shape)} dimensions instead of {len(shape)} ({got})"
    for axis, (have, need) in enumerate(zip(got_shape, shape)):
        if need is not None and have != int(need):
            return f"{expected}: dimension {axis} is {have}, not {int(need)} ({got})"
    numel = 1
    for e in got_shape:
        numel *= e
    if min_numel is not None and numel < int(min_numel):
        return f"{expected}: {numel} elements are too few ({got})"
    dense = 1
    for extent, stride in zip(reversed(got_shape), reversed(got_stride)):
        if numel and extent > 1 and stride != dense:  # (the stride of an extent-1 dimension is arbitrary in torch)
            return f"{expected}: it is a strided view ({got}) and nothing is copied here, the results are written in place; pass {name}.contiguous()"
        dense *= extent
    return None


def _device_complaint(name, t, device_index):
    """The other half: ``t`` lives in the memory of the context's HIP device (``device_index`` None: of any one HIP device)."""
    if not t.is_cuda:
        return f"{name} must be a CUDA tensor (got one on {t.device}): the kernels take its pointer, there is no host path and no copy here"
    if device_index is not None and t.device.index != device_index:
        return f"{name} must be on cuda:{device_index}, the device of the context and of the call's other tensors (got one on {t.device})"
    return None


def _check(name, t, dtypes, shape, device_index, min_numel=None):
    """Refuses (ValueError) a tensor argument the C ABI would misread; never copies or converts.  Every ``data_ptr()`` of this module
    is taken from a tensor that passed here (tests/test_device_args_cpu.py walks the entries and holds that)."""
    complaint = _tensor_complaint(name, t, dtypes, shape, min_numel) or _device_complaint(name, t, device_index)
    if complaint:
        raise ValueError(complaint)


def _call_device(ctx, first):
    """The device index a call's tensors must share: the context's where it is known (context_on_stream), else the first tensor's."""
    index = getattr(ctx, "device_index", None)
    if index is None and getattr(first, "is_cuda", False):
        index = first.device.index
    return index


def _check_pairs(n_ref, pred_uv, cur_uv, n_cur, device_index):
    """NearbyMatch's pixel arrays: float32 [n_ref, 2] and [n_cur, 2], both or neither."""
    if (pred_uv is None) != (cur_uv is None):
        raise ValueError(f"pred_uv and cur_uv go together: NearbyMatch needs both, ForceMatch neither (got {'pred_uv' if cur_uv is None else 'cur_uv'} alone)")
    if pred_uv is not None:
        _check("pred_uv", pred_uv, _F32, (n_ref, 2), device_index)
        _check("cur_uv", cur_uv, _F32, (n_cur, 2), device_index)


def context_on_stream(stream, device_index: Optional[int] = None) -> Context:
    """A context that launches on the given ``torch.cuda.Stream`` (not the legacy null stream), so
    torch events, collectives and allocations made under ``with torch.cuda.stream(stream)`` order
    correctly with the kernels."""
    torch = _torch()
    if device_index is None:
        device_index = stream.device.index if stream.device.index is not None else torch.cuda.current_device()
    handle = stream.cuda_stream
    if not handle:
        raise ValueError("pass a non-default torch.cuda.Stream (the null stream has no handle to borrow)")
    ctx = Context(device_index, handle)
    ctx.device_index = int(device_index)  # what the entries below hold their tensors to
    ctx.stream = stream  # KltVideoTracker orders torch's own work (allocations, the caller's stream) with the kernels through it
    return ctx


def pyramid_from_tensors(levels: Sequence, ctx: Context) -> ImagePyramid:
    """levels: uint8 CUDA tensors [rows, cols], contiguous.  Borrowed, not copied."""
    desc = []
    for k, t in enumerate(levels):
        _check(f"levels[{k}]", t, _U8, (None, None), _call_device(ctx, t))
        desc.append((t.data_ptr(), t.shape[0], t.shape[1]))
    return ImagePyramid.from_device_levels(desc, ctx, keepalive=list(levels))


def upload_pyramid(host_levels: Sequence[np.ndarray], ctx: Context, device) -> ImagePyramid:
    torch = _torch()
    tensors = [torch.from_numpy(np.ascontiguousarray(l)).to(device) for l in host_levels]
    return pyramid_from_tensors(tensors, ctx)


class DeviceKlt:
    """Runs one tracker variant on device-resident feature buffers.

    ``track(ref_uv, cur_uv_in, status_in, cur_uv_out, status_out, iters=None)`` enqueues ONE kernel on
    the context's stream and returns immediately; the out tensors may alias the in tensors.
    """

    def __init__(self, model: str, options: OpticalFlowOptions, ref_pyr: ImagePyramid, cur_pyr: ImagePyramid, ctx: Context,
                 prior: Optional[np.ndarray] = None, consider_luminance: bool = False, single_level: bool = False):
        self.model = N.MODELS[model]
        self.opt = options.to_native()
        self.ref_pyr, self.cur_pyr, self.ctx = ref_pyr, cur_pyr, ctx
        self.prior = None if prior is None else np.ascontiguousarray(prior, dtype=np.float32).reshape(4)
        self.lum = int(bool(consider_luminance))
        self.single = int(bool(single_level))

    def _check_in(self, ref_uv, cur_uv_in, status_in, iters=None):
        """ref_uv and cur_uv_in: float32 [n, 2]; status_in: uint8 [n]; iters: int32 [n] or None; all contiguous, on the context's device.
        Returns (n, that device's index)."""
        dev = _call_device(self.ctx, ref_uv)
        _check("ref_uv", ref_uv, _F32, (None, 2), dev)
        n = int(ref_uv.shape[0])
        _check("cur_uv_in", cur_uv_in, _F32, (n, 2), dev)
        _check("status_in", status_in, _U8, (n,), dev)
        if iters is not None:
            _check("iters", iters, _COUNTS, (n,), dev)
        return n, dev

    @staticmethod
    def _check_out(n, dev, cur_uv_out, status_out):
        """cur_uv_out: float32 [n, 2]; status_out: uint8 [n]; contiguous, on the device of the inputs (which they may alias)."""
        _check("cur_uv_out", cur_uv_out, _F32, (n, 2), dev)
        _check("status_out", status_out, _U8, (n,), dev)

    def _prior(self):
        return None if self.prior is None else self.prior.ctypes.data_as(C.c_void_p)

    def bind(self, ref_uv, cur_uv_in, status_in, cur_uv_out, status_out, iters=None):
        """Pre-marshals one launch on fixed buffers; the returned callable enqueues it with minimal
        host work (for launch-rate-sensitive loops).  The tensors must outlive the callable.
        Tensors: contiguous float32 [n, 2] pairs, uint8 [n] status, int32 [n] iters, as ``track``; checked here once, not per launch."""
        n, dev = self._check_in(ref_uv, cur_uv_in, status_in, iters)
        self._check_out(n, dev, cur_uv_out, status_out)
        fn = N.lib().ftk_klt_track_device
        args = (self.ctx.handle, self.model, C.byref(self.opt), self.ref_pyr.handle, self.cur_pyr.handle, C.c_void_p(ref_uv.data_ptr()),
                C.c_void_p(cur_uv_in.data_ptr()), C.c_void_p(cur_uv_out.data_ptr()), C.c_void_p(status_in.data_ptr()),
                C.c_void_p(status_out.data_ptr()), n, self._prior(), self.lum, self.single, None if iters is None else C.c_void_p(iters.data_ptr()))
        keep = (ref_uv, cur_uv_in, status_in, cur_uv_out, status_out, iters)
        handle = self.ctx.handle

        def launch(_fn=fn, _args=args, _keep=keep):
            rc = _fn(*_args)
            if rc != 0:
                N.check(rc, handle)

        return launch

    @property
    def max_track_points(self) -> int:
        """kMaxTrackPointsNumber of this tracker's options (the GLOBAL cap when the feature list is sharded)."""
        return int(self.opt.max_track_points)

    def track_sharded(self, comm: "Comm", ref_uv, cur_uv_in, status_in, cur_uv_out, status_out, iters=None):
        """ftk_klt_track_sharded_device: this rank's block of the (full-length) buffers, RCCL all-gather, scatter — every rank's
        out tensors hold all n results afterwards (stream-ordered).
        Tensors: contiguous float32 [n, 2] pairs, uint8 [n] status, int32 [n] iters (only this rank's block is written), as ``track``."""
        n, dev = self._check_in(ref_uv, cur_uv_in, status_in, iters)
        self._check_out(n, dev, cur_uv_out, status_out)
        rc = N.lib().ftk_klt_track_sharded_device(
            self.ctx.handle, comm.handle, self.model, C.byref(self.opt), self.ref_pyr.handle, self.cur_pyr.handle, C.c_void_p(ref_uv.data_ptr()),
            C.c_void_p(cur_uv_in.data_ptr()), C.c_void_p(cur_uv_out.data_ptr()), C.c_void_p(status_in.data_ptr()), C.c_void_p(status_out.data_ptr()), n,
            self._prior(), self.lum, self.single, None if iters is None else C.c_void_p(iters.data_ptr()))
        N.check(rc, self.ctx.handle)

    def bind_sharded(self, comm: "Comm", ref_uv, cur_uv_in, status_in, cur_uv_out, status_out):
        """Pre-marshalled track_sharded on fixed buffers (launch-rate-sensitive loops, HIP-graph capture).
        Tensors: contiguous float32 [n, 2] pairs and uint8 [n] status, as ``track``; checked here once, not per launch."""
        n, dev = self._check_in(ref_uv, cur_uv_in, status_in)
        self._check_out(n, dev, cur_uv_out, status_out)
        fn = N.lib().ftk_klt_track_sharded_device
        args = (self.ctx.handle, comm.handle, self.model, C.byref(self.opt), self.ref_pyr.handle, self.cur_pyr.handle, C.c_void_p(ref_uv.data_ptr()),
                C.c_void_p(cur_uv_in.data_ptr()), C.c_void_p(cur_uv_out.data_ptr()), C.c_void_p(status_in.data_ptr()), C.c_void_p(status_out.data_ptr()), n,
                self._prior(), self.lum, self.single, None)
        keep = (comm, ref_uv, cur_uv_in, status_in, cur_uv_out, status_out)
        handle = self.ctx.handle

        def launch(_fn=fn, _args=args, _keep=keep):
            rc = _fn(*_args)
            if rc != 0:
                N.check(rc, handle)

        return launch

    def track_shard(self, rank: int, world: int, ref_uv, cur_uv_in, status_in, packed_shard, iters=None):
        """ftk_klt_track_shard_device: rank's block tracked into its packed shard (for callers with their own collective).
        Tensors: inputs as ``track`` (full length n); packed_shard: contiguous uint8, at least ftk_klt_shard_bytes(n, world) bytes."""
        n, dev = self._check_in(ref_uv, cur_uv_in, status_in, iters)
        _check("packed_shard", packed_shard, _U8, (None,), dev, min_numel=N.lib().ftk_klt_shard_bytes(n, int(world)))
        rc = N.lib().ftk_klt_track_shard_device(
            self.ctx.handle, int(rank), int(world), self.model, C.byref(self.opt), self.ref_pyr.handle, self.cur_pyr.handle, C.c_void_p(ref_uv.data_ptr()),
            C.c_void_p(cur_uv_in.data_ptr()), C.c_void_p(status_in.data_ptr()), n, self._prior(), self.lum, self.single, C.c_void_p(packed_shard.data_ptr()),
            None if iters is None else C.c_void_p(iters.data_ptr()))
        N.check(rc, self.ctx.handle)

    def unpack_shards(self, gathered, n: int, world: int, cur_uv_out, status_out):
        """ftk_klt_unpack_shards_device: the scatter of ``world`` gathered shards into the n results.
        Tensors: gathered: contiguous uint8, at least world * ftk_klt_shard_bytes(n, world) bytes; cur_uv_out: float32 [n, 2]; status_out: uint8 [n]."""
        n, world = int(n), int(world)
        dev = _call_device(self.ctx, gathered)
        _check("gathered", gathered, _U8, (None,), dev, min_numel=max(world, 0) * N.lib().ftk_klt_shard_bytes(n, world))
        self._check_out(n, dev, cur_uv_out, status_out)
        N.check(N.lib().ftk_klt_unpack_shards_device(self.ctx.handle, C.c_void_p(gathered.data_ptr()), n, world, C.c_void_p(cur_uv_out.data_ptr()),
                                                     C.c_void_p(status_out.data_ptr())), self.ctx.handle)

    def track(self, ref_uv, cur_uv_in, status_in, cur_uv_out, status_out, iters=None, max_track_points=None):
        """``max_track_points`` overrides the options' cap for this launch (a shard's share of the global cap).
        Tensors: ref_uv, cur_uv_in, cur_uv_out: contiguous float32 [n, 2]; status_in, status_out: uint8 [n]; iters: int32 [n] or None; the
        out tensors may alias the in tensors.  A strided view, another dtype or a short buffer is a ValueError, never a copy.
        Every element of cur_uv_out, status_out and iters is written: a feature that arrives with a status above tracked, or lies beyond
        the cap, gets its cur_uv_in and status_in copied and 0 iterations, so nothing depends on what the out tensors held."""
        n, dev = self._check_in(ref_uv, cur_uv_in, status_in, iters)
        self._check_out(n, dev, cur_uv_out, status_out)
        opt = self.opt
        if max_track_points is not None and int(max_track_points) != int(opt.max_track_points):
            opt = N.KltOptions.from_buffer_copy(self.opt)
            opt.max_track_points = int(max_track_points)
        rc = N.lib().ftk_klt_track_device(
            self.ctx.handle, self.model, C.byref(opt), self.ref_pyr.handle, self.cur_pyr.handle, C.c_void_p(ref_uv.data_ptr()),
            C.c_void_p(cur_uv_in.data_ptr()), C.c_void_p(cur_uv_out.data_ptr()), C.c_void_p(status_in.data_ptr()),
            C.c_void_p(status_out.data_ptr()), n, self._prior(), self.lum, self.single, None if iters is None else C.c_void_p(iters.data_ptr()))
        N.check(rc, self.ctx.handle)


class Comm:
    """ftk_comm: the communicator of the native multi-GPU path (one process per GPU; RCCL all-gather issued by libftk_hip.so on
    the context's stream).  ``unique_id`` (128 bytes from ``Comm.unique_id()`` on rank 0, handed to the other ranks by any
    means) is required for world > 1; world == 1 with no id needs no RCCL."""

    def __init__(self, ctx: Context, rank: int = 0, world: int = 1, unique_id: Optional[bytes] = None):
        self.ctx, self.rank, self.world = ctx, int(rank), int(world)
        out = C.c_void_p()
        buf = None if unique_id is None else C.create_string_buffer(bytes(unique_id), N.UNIQUE_ID_BYTES)
        N.check(N.lib().ftk_comm_create(ctx.handle, self.rank, self.world, buf, C.byref(out)), ctx.handle)
        self._handle = out

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(N.UNIQUE_ID_BYTES)
        N.check(N.lib().ftk_comm_unique_id(buf), None)
        return buf.raw

    @property
    def handle(self):
        return self._handle

    def close(self):
        if self._handle:
            library = N.loaded()  # (as Context.close)
            if library is not None:
                library.ftk_comm_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_bounds(n: int, world: int, rank: int):
    """ftk_shard_bounds: the native twin of feature_tracker_amd.dist.shard_bounds."""
    b, e = C.c_int32(), C.c_int32()
    N.lib().ftk_shard_bounds(n, world, rank, C.byref(b), C.byref(e))
    return b.value, e.value


def _check_words(ctx, ref_words, cur_words, n_bits, index_pairs, pred_uv, cur_uv):
    """Packed descriptors: int32 / uint32 [n_ref, words] and [n_cur, words], n_bits <= 32 * words; index_pairs: int32 [n_ref]."""
    dev = _call_device(ctx, ref_words)
    _check("ref_words", ref_words, _WORDS, (None, None), dev)
    n_ref, words = int(ref_words.shape[0]), int(ref_words.shape[1])
    _check("cur_words", cur_words, _WORDS, (None, words), dev)
    n_cur = int(cur_words.shape[0])
    if int(n_bits) > 32 * words:
        raise ValueError(f"n_bits {int(n_bits)} exceeds the {words} words (= {32 * words} bits) of a row of ref_words / cur_words")
    _check("index_pairs", index_pairs, _I32, (n_ref,), dev)
    _check_pairs(n_ref, pred_uv, cur_uv, n_cur, dev)
    return n_ref, n_cur, words, dev


def hamming_match_sharded_device(ctx: Context, comm: Comm, ref_words, cur_words, n_bits: int, max_distance: float, index_pairs, pred_uv=None,
                                 cur_uv=None, max_col: int = 40, max_row: int = 40):
    """ftk_hamming_match_sharded_device on torch tensors: every rank passes ALL reference rows; index_pairs is complete everywhere.
    Tensors, all contiguous: words int32 / uint32 [n_ref, words] and [n_cur, words]; index_pairs int32 [n_ref]; pred_uv / cur_uv float32 [n_ref, 2] / [n_cur, 2]."""
    n_ref, n_cur, words, _ = _check_words(ctx, ref_words, cur_words, n_bits, index_pairs, pred_uv, cur_uv)
    rc = N.lib().ftk_hamming_match_sharded_device(
        ctx.handle, comm.handle, C.c_void_p(ref_words.data_ptr()), n_ref, C.c_void_p(cur_words.data_ptr()), n_cur,
        words, int(n_bits), float(max_distance), None if pred_uv is None else C.c_void_p(pred_uv.data_ptr()),
        None if cur_uv is None else C.c_void_p(cur_uv.data_ptr()), int(max_col), int(max_row), C.c_void_p(index_pairs.data_ptr()))
    N.check(rc, ctx.handle)


def hamming_match_device(ctx: Context, ref_words, cur_words, n_bits: int, max_distance: float, index_pairs, pred_uv=None, cur_uv=None,
                         max_col: int = 40, max_row: int = 40, workspace=None):
    """ForceMatch (pred_uv None) / NearbyMatch on packed descriptors held in CUDA tensors.
    Tensors, all contiguous: words int32 / uint32 [n_ref, words] and [n_cur, words] (same words, n_bits <= 32 * words); index_pairs int32
    [n_ref] (in/out); pred_uv / cur_uv float32 [n_ref, 2] / [n_cur, 2], both or neither; workspace int64 / uint64, at least n_ref elements, or None."""
    n_ref, n_cur, words, dev = _check_words(ctx, ref_words, cur_words, n_bits, index_pairs, pred_uv, cur_uv)
    if workspace is not None:
        _check("workspace", workspace, _KEYS, (None,), dev, min_numel=n_ref)
    rc = N.lib().ftk_hamming_match_device(
        ctx.handle, C.c_void_p(ref_words.data_ptr()), n_ref, C.c_void_p(cur_words.data_ptr()), n_cur,
        words, int(n_bits), float(max_distance), None if pred_uv is None else C.c_void_p(pred_uv.data_ptr()),
        None if cur_uv is None else C.c_void_p(cur_uv.data_ptr()), int(max_col), int(max_row), C.c_void_p(index_pairs.data_ptr()),
        None if workspace is None else C.c_void_p(workspace.data_ptr()))
    N.check(rc, ctx.handle)


def cosine_match_device(ctx: Context, ref_desc, cur_desc, max_distance: float, index_pairs, pred_uv=None, cur_uv=None, max_col: int = 40,
                        max_row: int = 40):
    """ForceMatch (pred_uv None) / NearbyMatch on float descriptors held in CUDA tensors.
    Tensors, all contiguous: descriptors float32 [n_ref, dim] and [n_cur, dim], one row per feature (a [dim, n] network output: pass
    ``desc.t().contiguous()``); index_pairs int32 [n_ref] (in/out); pred_uv / cur_uv float32 [n_ref, 2] / [n_cur, 2], both or neither."""
    dev = _call_device(ctx, ref_desc)
    _check("ref_desc", ref_desc, _F32, (None, None), dev)
    n_ref, dim = int(ref_desc.shape[0]), int(ref_desc.shape[1])
    _check("cur_desc", cur_desc, _F32, (None, dim), dev)
    n_cur = int(cur_desc.shape[0])
    _check("index_pairs", index_pairs, _I32, (n_ref,), dev)
    _check_pairs(n_ref, pred_uv, cur_uv, n_cur, dev)
    rc = N.lib().ftk_cosine_match_device(
        ctx.handle, C.c_void_p(ref_desc.data_ptr()), n_ref, C.c_void_p(cur_desc.data_ptr()), n_cur,
        dim, float(max_distance), None if pred_uv is None else C.c_void_p(pred_uv.data_ptr()),
        None if cur_uv is None else C.c_void_p(cur_uv.data_ptr()), int(max_col), int(max_row), C.c_void_p(index_pairs.data_ptr()))
    N.check(rc, ctx.handle)


def brief_compute_device(ctx: Context, image_pyr: ImagePyramid, uv, n_bits: int, half_patch: int, words_out, level: int = 0):
    """BRIEF descriptors of CUDA-resident features straight into packed CUDA words.
    Tensors, contiguous: uv float32 [n, 2]; words_out int32 / uint32 [n, ceil(n_bits / 32)]."""
    dev = _call_device(ctx, uv)
    _check("uv", uv, _F32, (None, 2), dev)
    n = int(uv.shape[0])
    _check("words_out", words_out, _WORDS, (n, (max(int(n_bits), 0) + 31) // 32), dev)
    rc = N.lib().ftk_brief_compute_device(ctx.handle, image_pyr.handle, int(level), C.c_void_p(uv.data_ptr()), n, int(n_bits),
                                          int(half_patch), C.c_void_p(words_out.data_ptr()))
    N.check(rc, ctx.handle)


class DeviceDirectBatch:
    """A batch of DirectMethod pose problems (ftk_direct_track_batch_device): one workgroup per problem, ONE launch.
    Every tensor stays in HBM; ``problems`` is a list of dicts with keys ref, cur (ImagePyramid), K (4 floats),
    p_c_in_ref [n, 3], ref_uv [n, 2], cur_uv [n, 2] (in/out), pose [7] (q w,x,y,z then p; in/out), status [n] uint8,
    status_valid (bool) and optionally iterations (int32 [1]).
    Tensors: contiguous, float32 but for status and iterations, on the context's device; checked once, here, where their pointers are taken."""

    def __init__(self, options, problems, ctx: Context):
        self.ctx = ctx
        self.opt = options.to_native()
        self._keep = problems
        self.n = len(problems)
        self.table = (N.DirectProblem * self.n)()
        for k, pr in enumerate(problems):
            t = self.table[k]
            where = f"problems[{k}]"
            dev = _call_device(ctx, pr["ref_uv"])
            _check(f"{where}['ref_uv']", pr["ref_uv"], _F32, (None, 2), dev)
            n = int(pr["ref_uv"].shape[0])
            _check(f"{where}['p_c_in_ref']", pr["p_c_in_ref"], _F32, (n, 3), dev)
            _check(f"{where}['cur_uv']", pr["cur_uv"], _F32, (n, 2), dev)
            _check(f"{where}['pose']", pr["pose"], _F32, (7,), dev)
            _check(f"{where}['status']", pr["status"], _U8, (n,), dev)
            it = pr.get("iterations")
            if it is not None:
                _check(f"{where}['iterations']", it, _COUNTS, (1,), dev)
            t.ref, t.cur = pr["ref"].handle, pr["cur"].handle
            for i in range(4):
                t.K[i] = float(pr["K"][i])
            t.d_p_c_in_ref = pr["p_c_in_ref"].data_ptr()
            t.d_ref_uv = pr["ref_uv"].data_ptr()
            t.d_cur_uv = pr["cur_uv"].data_ptr()
            t.n = n
            t.d_pose = pr["pose"].data_ptr()
            t.d_status = pr["status"].data_ptr()
            t.status_valid = int(bool(pr.get("status_valid", False)))
            t.d_iterations = None if it is None else it.data_ptr()

    def track(self):
        N.check(N.lib().ftk_direct_track_batch_device(self.ctx.handle, C.byref(self.opt), self.table, self.n), self.ctx.handle)


def dense_flow_device(ctx: Context, options, ref_pyr: ImagePyramid, cur_pyr: ImagePyramid, flow_r, flow_c, k_moments=(0.0, 0.0, 0.0)) -> None:
    """ftk_dense_flow_device: Farneback dense flow of the two pyramids into ``flow_r`` / ``flow_c`` (contiguous float32 CUDA tensors of
    level 0's ref shape), enqueued on the context's stream; no synchronisation, capturable once an uncaptured call of the same shape
    and half patch has made the workspace resident.  ``options``: a DenseOpticalFlowOptions or a native DenseFlowOptions;
    ``k_moments`` are the k2 / k4 / k22 a half patch of 0 uses."""
    from .tracker import DenseOpticalFlowOptions

    opt = options.to_native(k_moments) if isinstance(options, DenseOpticalFlowOptions) else options
    _, rows, cols = ref_pyr.level_desc(0)
    dev = _call_device(ctx, flow_r)
    _check("flow_r", flow_r, _F32, (rows, cols), dev)
    _check("flow_c", flow_c, _F32, (rows, cols), dev)
    rc = N.lib().ftk_dense_flow_device(ctx.handle, C.byref(opt), ref_pyr.handle, cur_pyr.handle, C.c_void_p(flow_r.data_ptr()),
                                       C.c_void_p(flow_c.data_ptr()))
    N.check(rc, ctx.handle)


def _corr_check(name, t, dim):
    """A contiguous float32 CUDA tensor of ``dim`` dimensions (the correlation entries take their stream, hence their device, from torch)."""
    _check(name, t, _F32, (None,) * dim, None)


def corr_pyramid_build_device(ctx: Context, fmap0, fmap1, levels: int, volume, stream=None) -> None:
    """ftk_corr_pyramid_build_device: the correlation pyramid of ``fmap0`` / ``fmap1`` (contiguous float32 CUDA [B, C, H, W]) into
    ``volume`` (contiguous float32 CUDA, ftk_corr_pyramid_layout's element count), enqueued on ``stream`` (a torch.cuda.Stream; default:
    torch's current stream).  No synchronisation, no allocation: capturable."""
    _torch()  # (no HIP device: that refusal comes first)
    _corr_check("fmap0", fmap0, 4)
    _corr_check("fmap1", fmap1, 4)
    if tuple(fmap0.shape) != tuple(fmap1.shape) or fmap0.device != fmap1.device:
        raise ValueError(f"fmap0 and fmap1 differ: {tuple(fmap0.shape)} on {fmap0.device} vs {tuple(fmap1.shape)} on {fmap1.device}")
    B, Cc, H, W = fmap0.shape
    elements, _, _ = N.corr_pyramid_layout(B, H, W, levels)
    _corr_check("volume", volume, volume.dim())
    if volume.numel() != elements or volume.device != fmap0.device:
        raise ValueError(f"volume must hold {elements} floats on {fmap0.device} (got {volume.numel()} on {volume.device})")
    s = stream_or_current(fmap0, stream)
    rc = N.lib().ftk_corr_pyramid_build_device(ctx.handle, C.c_void_p(s.cuda_stream), C.c_void_p(fmap0.data_ptr()), C.c_void_p(fmap1.data_ptr()),
                                               B, Cc, H, W, int(levels), C.c_void_p(volume.data_ptr()))
    N.check(rc, ctx.handle)


def corr_pyramid_lookup_device(ctx: Context, volume, levels: int, radius: int, coords, out, per_level: bool = False, stream=None) -> None:
    """ftk_corr_pyramid_lookup_device: the (2r+1)^2 windows of every level around ``coords`` (contiguous float32 CUDA [B, 2, H, W], x then y)
    into ``out``: [B, levels * K, H, W], or with ``per_level`` ``levels`` consecutive [B, H, W, K] blocks (K = (2r+1)^2)."""
    _torch()  # (no HIP device: that refusal comes first)
    _corr_check("coords", coords, 4)
    B, two, H, W = coords.shape
    if two != 2:
        raise ValueError(f"coords must be [B, 2, H, W] (got {tuple(coords.shape)})")
    elements, _, _ = N.corr_pyramid_layout(B, H, W, levels)
    _corr_check("volume", volume, volume.dim())
    if volume.numel() != elements or volume.device != coords.device:
        raise ValueError(f"volume must hold {elements} floats on {coords.device} (got {volume.numel()} on {volume.device})")
    K = (2 * int(radius) + 1) ** 2
    _corr_check("out", out, out.dim())
    if out.numel() != B * levels * K * H * W or out.device != coords.device:
        raise ValueError(f"out must hold {B * levels * K * H * W} floats on {coords.device}")
    s = stream_or_current(coords, stream)
    rc = N.lib().ftk_corr_pyramid_lookup_device(ctx.handle, C.c_void_p(s.cuda_stream), C.c_void_p(volume.data_ptr()), B, H, W, int(levels),
                                                int(radius), C.c_void_p(coords.data_ptr()), C.c_void_p(out.data_ptr()), int(bool(per_level)))
    N.check(rc, ctx.handle)


from ._device_flow_upsample import flow_upsample_device  # noqa: E402,F401  (RAFT's UpsampleFlow; its own file, see there)
from ._device_flow_points import flow_track_points_device  # noqa: E402,F401  (sparse tracking from RAFT's coarse flow; its own file, see there)
from ._device_flow_warm import flow_warm_device  # noqa: E402,F401  (the warm start of RAFT on video; its own file, see there)
from ._device_sep_conv_gru import sep_conv_gru_device  # noqa: E402,F401  (RAFT's SepConvGru; its own file, see there)
from ._device_raft_conv import channel_normalise_device, conv2d_device, conv2d_pool_device, conv2d_strided_device  # noqa: E402,F401  (the stock layers of RAFT's UpdateBlock and SuperPoint's; its own file, see there)
from ._device_corr_ondemand import corr_ondemand_lookup_device, corr_ondemand_prepare_device  # noqa: E402,F401  (RAFT's on-demand correlation; its own file, see there)
from ._device_klt_video import _check_bound, harris_detect_device, track_table_fill_device, track_table_retire_device  # noqa: E402,F401  (masked Harris detection and KltVideoTracker's table; its own file, see there)
from ._device_epipolar import epipolar_ransac_device  # noqa: E402,F401  (two-view outlier rejection; its own file, see there)
from ._device_two_view import two_view_ransac_device  # noqa: E402,F401  (the same with a choice of model)
from ._device_two_view_pose import two_view_pose_device  # noqa: E402,F401  (the pose and the landmarks of the inliers; its own file, see there)
from ._device_pnp import pnp_ransac_device, pnp_ransac_sampled_device  # noqa: E402,F401  (the pose from landmarks and their pixels; its own file, see there)
from ._device_landmark_table import landmark_table_begin_device, landmark_table_end_device  # noqa: E402,F401  (the landmark table; its own file, see there)
from ._device_keypoint_decode import keypoint_decode_device  # noqa: E402,F401  (the keypoint decoder; its own file, see there)
from ._device_match_assignment import match_assignment_device  # noqa: E402,F401  (LightGlue's assignment head; its own file, see there)
from ._device_match_table import match_table_query_device, match_table_update_device  # noqa: E402,F401  (MatchVideoTracker's landmark table; its own file, see there)
from ._device_transformer import attention_device, linear_device, transformer_layer_device  # noqa: E402,F401  (LightGlue's transformer layer; likewise)
from ._device_lightglue_adaptive import (lightglue_adapt_step_device, lightglue_confidence_device, lightglue_finish_device,  # noqa: E402,F401
                                         transformer_layer_adaptive_device)  # (LightGlue's adaptive depth and width; likewise)


def _nn_stream(tensor, stream):
    return C.c_void_p(stream_or_current(tensor, stream).cuda_stream)


def nn_match_scores_device(ctx: Context, scores, min_score: float, match_index, status, stream=None) -> None:
    """ftk_nn_match_scores_device: mutual-best matching of ``scores`` (float32 CUDA [B, n_ref, n_cur], any row / batch stride, unit column
    stride) into ``match_index`` (contiguous int32 [B, n_ref]) and ``status`` (contiguous uint8 [B, n_ref]), enqueued on ``stream``
    (default: torch's current stream).  No synchronisation; no allocation once the context's key workspace holds the size: capturable."""
    torch = _torch()
    if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32 or not scores.is_cuda or scores.dim() != 3:
        raise ValueError("scores must be a 3-D float32 CUDA tensor [B, n_ref, n_cur] (no CPU fallback, no other dtype)")
    B, n_ref, n_cur = scores.shape
    if n_cur > 1 and scores.stride(2) != 1:
        raise ValueError(f"scores must have unit column stride (got strides {tuple(scores.stride())}): pass a row / batch slice, or .contiguous()")
    for name, t, dt in (("match_index", match_index, torch.int32), ("status", status, torch.uint8)):
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (B, n_ref) or t.device != scores.device:
            raise ValueError(f"{name} must be a contiguous {dt} tensor of shape ({B}, {n_ref}) on {scores.device}")
    # a size-1 dimension's stride is arbitrary in torch: give the extent the library validates against
    row_stride = scores.stride(1) if n_ref > 1 else max(n_cur, 1)
    batch_stride = scores.stride(0) if B > 1 else 0
    rc = N.lib().ftk_nn_match_scores_device(ctx.handle, _nn_stream(scores, stream), C.c_void_p(scores.data_ptr()), B, n_ref, n_cur,
                                            row_stride, batch_stride, float(min_score), C.c_void_p(match_index.data_ptr()),
                                            C.c_void_p(status.data_ptr()))
    N.check(rc, ctx.handle)


def nn_match_list_device(ctx: Context, matches, n_ref: int, n_cur: int, match_index, status, stream=None) -> None:
    """ftk_nn_match_list_device: ``matches`` (contiguous int64 CUDA [K, 2] rows of (idx_ref, idx_cur)) into ``match_index`` (int32 [n_ref])
    and ``status`` (uint8 [n_ref]); the last applied row of an idx_ref wins."""
    torch = _torch()
    if not isinstance(matches, torch.Tensor) or matches.dtype != torch.int64 or not matches.is_cuda or matches.dim() != 2 or matches.size(1) != 2 \
            or not matches.is_contiguous():
        raise ValueError("matches must be a contiguous int64 CUDA tensor [K, 2]")
    for name, t, dt in (("match_index", match_index, torch.int32), ("status", status, torch.uint8)):
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (int(n_ref),) or t.device != matches.device:
            raise ValueError(f"{name} must be a contiguous {dt} tensor of shape ({n_ref},) on {matches.device}")
    rc = N.lib().ftk_nn_match_list_device(ctx.handle, _nn_stream(matches, stream), C.c_void_p(matches.data_ptr()), matches.size(0),
                                          int(n_ref), int(n_cur), C.c_void_p(match_index.data_ptr()), C.c_void_p(status.data_ptr()))
    N.check(rc, ctx.handle)


def nn_fill_pixels_device(ctx: Context, match_index, cur_uv, matched_uv, stream=None) -> None:
    """ftk_nn_fill_pixels_device: ``matched_uv`` (float32 [n_cur, 2]) = ``cur_uv`` with entry t < n_ref replaced by cur_uv[match_index[t]]
    where that index is valid (``match_index``: int32 [n_ref])."""
    torch = _torch()
    n_ref, n_cur = match_index.numel(), cur_uv.size(0)
    if match_index.dtype != torch.int32 or not match_index.is_cuda or not match_index.is_contiguous() or match_index.dim() != 1:
        raise ValueError("match_index must be a contiguous 1-D int32 CUDA tensor")
    for name, t in (("cur_uv", cur_uv), ("matched_uv", matched_uv)):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (n_cur, 2) or t.device != match_index.device:
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape ({n_cur}, 2) on {match_index.device}")
    rc = N.lib().ftk_nn_fill_pixels_device(ctx.handle, _nn_stream(match_index, stream), C.c_void_p(match_index.data_ptr()), n_ref,
                                           C.c_void_p(cur_uv.data_ptr()), n_cur, C.c_void_p(matched_uv.data_ptr()))
    N.check(rc, ctx.handle)
