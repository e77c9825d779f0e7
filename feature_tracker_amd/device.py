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
from .tracker import Context, ImagePyramid, OpticalFlowOptions


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("feature_tracker_amd.device needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch


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
    return Context(device_index, handle)


def pyramid_from_tensors(levels: Sequence, ctx: Context) -> ImagePyramid:
    """levels: uint8 CUDA tensors [rows, cols], contiguous.  Borrowed, not copied."""
    desc = []
    for t in levels:
        if t.dtype.__str__() != "torch.uint8" or not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
            raise ValueError("pyramid levels must be contiguous 2-D uint8 CUDA tensors")
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

    def bind(self, ref_uv, cur_uv_in, status_in, cur_uv_out, status_out, iters=None):
        """Pre-marshals one launch on fixed buffers; the returned callable enqueues it with minimal
        host work (for launch-rate-sensitive loops).  The tensors must outlive the callable."""
        fn = N.lib().ftk_klt_track_device
        args = (self.ctx.handle, self.model, C.byref(self.opt), self.ref_pyr.handle, self.cur_pyr.handle, C.c_void_p(ref_uv.data_ptr()),
                C.c_void_p(cur_uv_in.data_ptr()), C.c_void_p(cur_uv_out.data_ptr()), C.c_void_p(status_in.data_ptr()),
                C.c_void_p(status_out.data_ptr()), ref_uv.shape[0], None if self.prior is None else self.prior.ctypes.data_as(C.c_void_p),
                self.lum, self.single, None if iters is None else C.c_void_p(iters.data_ptr()))
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

    def _args(self, ref_uv, cur_uv_in, status_in):
        return (C.c_void_p(ref_uv.data_ptr()), C.c_void_p(cur_uv_in.data_ptr()), C.c_void_p(status_in.data_ptr()))

    def track_sharded(self, comm: "Comm", ref_uv, cur_uv_in, status_in, cur_uv_out, status_out, iters=None):
        """ftk_klt_track_sharded_device: this rank's block of the (full-length) buffers, RCCL all-gather, scatter — every rank's
        out tensors hold all n results afterwards (stream-ordered)."""
        r, c, s = self._args(ref_uv, cur_uv_in, status_in)
        rc = N.lib().ftk_klt_track_sharded_device(
            self.ctx.handle, comm.handle, self.model, C.byref(self.opt), self.ref_pyr.handle, self.cur_pyr.handle, r, c, C.c_void_p(cur_uv_out.data_ptr()),
            s, C.c_void_p(status_out.data_ptr()), ref_uv.shape[0], None if self.prior is None else self.prior.ctypes.data_as(C.c_void_p), self.lum, self.single,
            None if iters is None else C.c_void_p(iters.data_ptr()))
        N.check(rc, self.ctx.handle)

    def bind_sharded(self, comm: "Comm", ref_uv, cur_uv_in, status_in, cur_uv_out, status_out):
        """Pre-marshalled track_sharded on fixed buffers (launch-rate-sensitive loops, HIP-graph capture)."""
        r, c, s = self._args(ref_uv, cur_uv_in, status_in)
        fn = N.lib().ftk_klt_track_sharded_device
        args = (self.ctx.handle, comm.handle, self.model, C.byref(self.opt), self.ref_pyr.handle, self.cur_pyr.handle, r, c, C.c_void_p(cur_uv_out.data_ptr()), s,
                C.c_void_p(status_out.data_ptr()), ref_uv.shape[0], None if self.prior is None else self.prior.ctypes.data_as(C.c_void_p), self.lum, self.single, None)
        keep = (comm, ref_uv, cur_uv_in, status_in, cur_uv_out, status_out)
        handle = self.ctx.handle

        def launch(_fn=fn, _args=args, _keep=keep):
            rc = _fn(*_args)
            if rc != 0:
                N.check(rc, handle)

        return launch

    def track_shard(self, rank: int, world: int, ref_uv, cur_uv_in, status_in, packed_shard, iters=None):
        """ftk_klt_track_shard_device: rank's block tracked into its packed shard (for callers with their own collective)."""
        r, c, s = self._args(ref_uv, cur_uv_in, status_in)
        rc = N.lib().ftk_klt_track_shard_device(
            self.ctx.handle, int(rank), int(world), self.model, C.byref(self.opt), self.ref_pyr.handle, self.cur_pyr.handle, r, c, s, ref_uv.shape[0],
            None if self.prior is None else self.prior.ctypes.data_as(C.c_void_p), self.lum, self.single, C.c_void_p(packed_shard.data_ptr()),
            None if iters is None else C.c_void_p(iters.data_ptr()))
        N.check(rc, self.ctx.handle)

    def unpack_shards(self, gathered, n: int, world: int, cur_uv_out, status_out):
        N.check(N.lib().ftk_klt_unpack_shards_device(self.ctx.handle, C.c_void_p(gathered.data_ptr()), int(n), int(world), C.c_void_p(cur_uv_out.data_ptr()),
                                                     C.c_void_p(status_out.data_ptr())), self.ctx.handle)

    def track(self, ref_uv, cur_uv_in, status_in, cur_uv_out, status_out, iters=None, max_track_points=None):
        """``max_track_points`` overrides the options' cap for this launch (a shard's share of the global cap)."""
        n = ref_uv.shape[0]
        opt = self.opt
        if max_track_points is not None and int(max_track_points) != int(opt.max_track_points):
            opt = N.KltOptions.from_buffer_copy(self.opt)
            opt.max_track_points = int(max_track_points)
        rc = N.lib().ftk_klt_track_device(
            self.ctx.handle, self.model, C.byref(opt), self.ref_pyr.handle, self.cur_pyr.handle, C.c_void_p(ref_uv.data_ptr()),
            C.c_void_p(cur_uv_in.data_ptr()), C.c_void_p(cur_uv_out.data_ptr()), C.c_void_p(status_in.data_ptr()),
            C.c_void_p(status_out.data_ptr()), n, None if self.prior is None else self.prior.ctypes.data_as(C.c_void_p), self.lum, self.single,
            None if iters is None else C.c_void_p(iters.data_ptr()))
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
            N.lib().ftk_comm_destroy(self._handle)
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


def hamming_match_sharded_device(ctx: Context, comm: Comm, ref_words, cur_words, n_bits: int, max_distance: float, index_pairs, pred_uv=None,
                                 cur_uv=None, max_col: int = 40, max_row: int = 40):
    """ftk_hamming_match_sharded_device on torch tensors: every rank passes ALL reference rows; index_pairs is complete everywhere."""
    rc = N.lib().ftk_hamming_match_sharded_device(
        ctx.handle, comm.handle, C.c_void_p(ref_words.data_ptr()), ref_words.shape[0], C.c_void_p(cur_words.data_ptr()), cur_words.shape[0],
        ref_words.shape[1], int(n_bits), float(max_distance), None if pred_uv is None else C.c_void_p(pred_uv.data_ptr()),
        None if cur_uv is None else C.c_void_p(cur_uv.data_ptr()), int(max_col), int(max_row), C.c_void_p(index_pairs.data_ptr()))
    N.check(rc, ctx.handle)


def hamming_match_device(ctx: Context, ref_words, cur_words, n_bits: int, max_distance: float, index_pairs, pred_uv=None, cur_uv=None,
                         max_col: int = 40, max_row: int = 40, workspace=None):
    """ForceMatch (pred_uv None) / NearbyMatch on packed descriptors held in CUDA tensors ([n, words] int32/uint32)."""
    rc = N.lib().ftk_hamming_match_device(
        ctx.handle, C.c_void_p(ref_words.data_ptr()), ref_words.shape[0], C.c_void_p(cur_words.data_ptr()), cur_words.shape[0],
        ref_words.shape[1], int(n_bits), float(max_distance), None if pred_uv is None else C.c_void_p(pred_uv.data_ptr()),
        None if cur_uv is None else C.c_void_p(cur_uv.data_ptr()), int(max_col), int(max_row), C.c_void_p(index_pairs.data_ptr()),
        None if workspace is None else C.c_void_p(workspace.data_ptr()))
    N.check(rc, ctx.handle)


def cosine_match_device(ctx: Context, ref_desc, cur_desc, max_distance: float, index_pairs, pred_uv=None, cur_uv=None, max_col: int = 40,
                        max_row: int = 40):
    """ForceMatch (pred_uv None) / NearbyMatch on float descriptors held in CUDA tensors ([n, dim] float32, contiguous)."""
    rc = N.lib().ftk_cosine_match_device(
        ctx.handle, C.c_void_p(ref_desc.data_ptr()), ref_desc.shape[0], C.c_void_p(cur_desc.data_ptr()), cur_desc.shape[0],
        cur_desc.shape[1], float(max_distance), None if pred_uv is None else C.c_void_p(pred_uv.data_ptr()),
        None if cur_uv is None else C.c_void_p(cur_uv.data_ptr()), int(max_col), int(max_row), C.c_void_p(index_pairs.data_ptr()))
    N.check(rc, ctx.handle)


def brief_compute_device(ctx: Context, image_pyr: ImagePyramid, uv, n_bits: int, half_patch: int, words_out, level: int = 0):
    """BRIEF descriptors of CUDA-resident features straight into packed CUDA words ([n, ceil(n_bits/32)] int32)."""
    rc = N.lib().ftk_brief_compute_device(ctx.handle, image_pyr.handle, int(level), C.c_void_p(uv.data_ptr()), uv.shape[0], int(n_bits),
                                          int(half_patch), C.c_void_p(words_out.data_ptr()))
    N.check(rc, ctx.handle)


class DeviceDirectBatch:
    """A batch of DirectMethod pose problems (ftk_direct_track_batch_device): one workgroup per problem, ONE launch.
    Every tensor stays in HBM; ``problems`` is a list of dicts with keys ref, cur (ImagePyramid), K (4 floats),
    p_c_in_ref [n, 3], ref_uv [n, 2], cur_uv [n, 2] (in/out), pose [7] (q w,x,y,z then p; in/out), status [n] uint8,
    status_valid (bool) and optionally iterations (int32 [1])."""

    def __init__(self, options, problems, ctx: Context):
        self.ctx = ctx
        self.opt = options.to_native()
        self._keep = problems
        self.n = len(problems)
        self.table = (N.DirectProblem * self.n)()
        for k, pr in enumerate(problems):
            t = self.table[k]
            t.ref, t.cur = pr["ref"].handle, pr["cur"].handle
            for i in range(4):
                t.K[i] = float(pr["K"][i])
            t.d_p_c_in_ref = pr["p_c_in_ref"].data_ptr()
            t.d_ref_uv = pr["ref_uv"].data_ptr()
            t.d_cur_uv = pr["cur_uv"].data_ptr()
            t.n = int(pr["ref_uv"].shape[0])
            t.d_pose = pr["pose"].data_ptr()
            t.d_status = pr["status"].data_ptr()
            t.status_valid = int(bool(pr.get("status_valid", False)))
            it = pr.get("iterations")
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
    for t in (flow_r, flow_c):
        if str(t.dtype) != "torch.float32" or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (rows, cols):
            raise ValueError(f"flow planes must be contiguous float32 CUDA tensors of shape ({rows}, {cols})")
    rc = N.lib().ftk_dense_flow_device(ctx.handle, C.byref(opt), ref_pyr.handle, cur_pyr.handle, C.c_void_p(flow_r.data_ptr()),
                                       C.c_void_p(flow_c.data_ptr()))
    N.check(rc, ctx.handle)


def _corr_check(name, t, dim):
    if str(t.dtype) != "torch.float32" or not t.is_cuda or not t.is_contiguous() or t.dim() != dim:
        raise ValueError(f"{name} must be a contiguous {dim}-D float32 CUDA tensor (got {tuple(t.shape)}, {t.dtype}, {t.device})")


def corr_pyramid_build_device(ctx: Context, fmap0, fmap1, levels: int, volume, stream=None) -> None:
    """ftk_corr_pyramid_build_device: the correlation pyramid of ``fmap0`` / ``fmap1`` (contiguous float32 CUDA [B, C, H, W]) into
    ``volume`` (contiguous float32 CUDA, ftk_corr_pyramid_layout's element count), enqueued on ``stream`` (a torch.cuda.Stream; default:
    torch's current stream).  No synchronisation, no allocation: capturable."""
    torch = _torch()
    _corr_check("fmap0", fmap0, 4)
    _corr_check("fmap1", fmap1, 4)
    if tuple(fmap0.shape) != tuple(fmap1.shape) or fmap0.device != fmap1.device:
        raise ValueError(f"fmap0 and fmap1 differ: {tuple(fmap0.shape)} on {fmap0.device} vs {tuple(fmap1.shape)} on {fmap1.device}")
    B, Cc, H, W = fmap0.shape
    elements, _, _ = N.corr_pyramid_layout(B, H, W, levels)
    _corr_check("volume", volume, volume.dim())
    if volume.numel() != elements or volume.device != fmap0.device:
        raise ValueError(f"volume must hold {elements} floats on {fmap0.device} (got {volume.numel()} on {volume.device})")
    s = torch.cuda.current_stream(fmap0.device) if stream is None else stream
    rc = N.lib().ftk_corr_pyramid_build_device(ctx.handle, C.c_void_p(s.cuda_stream), C.c_void_p(fmap0.data_ptr()), C.c_void_p(fmap1.data_ptr()),
                                               B, Cc, H, W, int(levels), C.c_void_p(volume.data_ptr()))
    N.check(rc, ctx.handle)


def corr_pyramid_lookup_device(ctx: Context, volume, levels: int, radius: int, coords, out, per_level: bool = False, stream=None) -> None:
    """ftk_corr_pyramid_lookup_device: the (2r+1)^2 windows of every level around ``coords`` (contiguous float32 CUDA [B, 2, H, W], x then y)
    into ``out``: [B, levels * K, H, W], or with ``per_level`` ``levels`` consecutive [B, H, W, K] blocks (K = (2r+1)^2)."""
    torch = _torch()
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
    s = torch.cuda.current_stream(coords.device) if stream is None else stream
    rc = N.lib().ftk_corr_pyramid_lookup_device(ctx.handle, C.c_void_p(s.cuda_stream), C.c_void_p(volume.data_ptr()), B, H, W, int(levels),
                                                int(radius), C.c_void_p(coords.data_ptr()), C.c_void_p(out.data_ptr()), int(bool(per_level)))
    N.check(rc, ctx.handle)


def _nn_stream(torch, device, stream):
    s = torch.cuda.current_stream(device) if stream is None else stream
    return C.c_void_p(s.cuda_stream)


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
    rc = N.lib().ftk_nn_match_scores_device(ctx.handle, _nn_stream(torch, scores.device, stream), C.c_void_p(scores.data_ptr()), B, n_ref, n_cur,
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
    rc = N.lib().ftk_nn_match_list_device(ctx.handle, _nn_stream(torch, matches.device, stream), C.c_void_p(matches.data_ptr()), matches.size(0),
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
    rc = N.lib().ftk_nn_fill_pixels_device(ctx.handle, _nn_stream(torch, match_index.device, stream), C.c_void_p(match_index.data_ptr()), n_ref,
                                           C.c_void_p(cur_uv.data_ptr()), n_cur, C.c_void_p(matched_uv.data_ptr()))
    N.check(rc, ctx.handle)
