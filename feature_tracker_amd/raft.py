"""RAFT's two operators that are not stock torch layers, the correlation pyramid (src/nn_optical_flow_tracker/raft/
correlation_volumes.py:19-83) as a drop-in class and the convex flow upsampling (Raft.UpsampleFlow, model.py:48-64) as a function, and
its recurrent unit, the separable ConvGRU (gru.py:46-76), as a class that runs one step in four fused launches, and the update block
around it (update_block.py:16-67) as ``MotionEncoder`` and ``UpdateBlock``, whose nine stock convolutions are one more kernel family.

``CorrelationPyramid(fmap0, fmap1, num_levels, radius)`` keeps the reference's attributes (``num_levels``, ``radius``,
``correlation_pyramid``) and ``__call__``; ``lookup`` returns the fused ``[B, L*K, H, W]`` tensor that model.py:87-88 builds with
``cat`` / ``permute`` / ``contiguous``.  torch owns every buffer (one volume tensor, the levels are views into it) and the kernels
launch on ``torch.cuda.current_stream()`` at each call, so construction and lookups can be captured in ``torch.cuda.graph``.
``upsample_flow(flow, mask, mask_scale)`` is ``Raft.UpsampleFlow(flow, mask_scale * mask)`` in one launch.
``SepConvGru(x_channels, h_channels, kernel_size)`` holds the reference module's twelve tensors; ``gru(x, h)`` is its ``forward`` with
``x`` one tensor or up to three read in place of their ``cat``.
``UpdateBlock.from_state_dict(state, "update_block.")`` is called like the reference's module, ``(net, inp, correlation, flow) ->
(new_net, mask, delta_flow)``, in 13 launches with no ``cat``.
``FeatureEncoder`` / ``ContextEncoder`` (encoder.py:25-68) run their 17 / 18 layers on the same kernel family with a stride, a residual
epilogue and BatchNorm folded into the weights once, and ``Raft.from_state_dict(state, levels, radius)(ref_image, cur_image)`` is
model.py:66-97: the whole forward pass, the list of flow predictions, with every convolution on these kernels.
``OnDemandCorrelation`` is ``CorrelationPyramid`` without the volume: it keeps the two feature maps channel-last and computes the
correlation values a lookup reads when it reads them; ``Raft(..., correlation="on_demand")`` uses it.
``track_points_from_flow`` moves feature points by the bilinear sample of the upsampled flow without storing it and gives them a
TrackStatus, with an optional forward-backward check, in one launch; ``Raft.track_points`` is the model as a feature tracker on top of it
(DESIGN.md 5.17).
``warm_start_flow`` pushes a coarse flow forward along itself (upstream RAFT's ``forward_interpolate``, on the device), ``flow_init`` /
``return_flow`` pass the state of the refinement loop into and out of ``Raft``, and ``RaftVideoTracker`` runs the model over a frame
sequence with the previous frame's feature map kept and each pair started from the previous pair's flow.
Inference only, float32 only, and no CPU fallback.
"""
from __future__ import annotations

import math
from typing import List, Mapping

from . import _native as N
from . import device as D
from ._torch_call import context_of as _device_context
from ._torch_call import context_of_index as _context  # noqa: F401  (the name tests and scripts ask this module for)


def _check_no_grad(torch, *tensors, what: str = "CorrelationPyramid") -> None:
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError(f"{what} is inference only (no backward): run it under torch.no_grad() or pass tensors that do not "
                           "require grad")


class CorrelationPyramid:
    """correlation_volumes.py:19-34: the all-pairs correlation of two float32 CUDA feature maps [B, C, H, W] and its
    ``num_levels - 1`` 2x2 average pools, built on the device by the HIP kernels of raft_corr_kernels.hip."""

    def __init__(self, fmap0, fmap1, num_levels: int, radius: int):
        torch = D._torch()
        for name, t in (("fmap0", fmap0), ("fmap1", fmap1)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 4:
                raise ValueError(f"{name} must be a 4-D float32 CUDA tensor [B, C, H, W] (no CPU fallback, no other dtype)")
        if fmap0.size() != fmap1.size() or fmap0.device != fmap1.device:
            raise ValueError(f"fmap0 and fmap1 must have the same size and device: {tuple(fmap0.shape)} on {fmap0.device} vs "
                             f"{tuple(fmap1.shape)} on {fmap1.device}")
        _check_no_grad(torch, fmap0, fmap1)
        if not 0 <= int(radius) <= N.FTK_CORR_MAX_RADIUS:
            raise ValueError(f"radius {radius} outside 0 .. {N.FTK_CORR_MAX_RADIUS}")
        B, _, H, W = fmap0.shape
        try:
            elements, offsets, dims = N.corr_pyramid_layout(B, H, W, int(num_levels))
        except N.FtkError as e:
            raise ValueError(f"CorrelationPyramid of {H} x {W} feature maps with num_levels={num_levels}: {e}") from None
        self.num_levels = int(num_levels)
        self.radius = int(radius)
        self._shape = (B, H, W)
        self._device = fmap0.device
        self._ctx = _device_context(fmap0)
        self._volume = torch.empty(elements, dtype=torch.float32, device=fmap0.device)
        D.corr_pyramid_build_device(self._ctx, fmap0.contiguous(), fmap1.contiguous(), self.num_levels, self._volume)
        n = B * H * W
        # the reference's list of [B*H*W, 1, H_l, W_l] tensors: zero-copy views into the one volume
        self.correlation_pyramid: List = [self._volume[off:off + n * h * w].view(n, 1, h, w) for off, (h, w) in zip(offsets, dims)]

    def _coords(self, pixel_locations):
        torch = D._torch()
        if not isinstance(pixel_locations, torch.Tensor) or pixel_locations.dim() != 4 or pixel_locations.size(1) != 2:
            raise ValueError("The size of pixel_locations should be [batch_size, 2, height, width].")
        B, H, W = self._shape
        if tuple(pixel_locations.shape) != (B, 2, H, W):
            raise ValueError(f"pixel_locations must be [{B}, 2, {H}, {W}] for this pyramid (got {tuple(pixel_locations.shape)})")
        if pixel_locations.dtype != torch.float32 or pixel_locations.device != self._device:
            raise ValueError(f"pixel_locations must be float32 on {self._device} (got {pixel_locations.dtype} on {pixel_locations.device})")
        _check_no_grad(torch, pixel_locations)
        return pixel_locations.contiguous()

    def __call__(self, pixel_locations):
        """correlation_volumes.py:48-77: per level a contiguous [B, H, W, (2r+1)^2] tensor of the bilinear window samples."""
        torch = D._torch()
        coords = self._coords(pixel_locations)
        B, H, W = self._shape
        K = (2 * self.radius + 1) ** 2
        block = B * H * W * K
        out = torch.empty(self.num_levels * block, dtype=torch.float32, device=self._device)
        D.corr_pyramid_lookup_device(self._ctx, self._volume, self.num_levels, self.radius, coords, out, per_level=True)
        return [out[l * block:(l + 1) * block].view(B, H, W, K) for l in range(self.num_levels)]

    def lookup(self, pixel_locations):
        """``torch.cat(self(pixel_locations), -1).permute(0, 3, 1, 2).contiguous()`` (model.py:87-88) in one launch: [B, L*K, H, W]."""
        torch = D._torch()
        coords = self._coords(pixel_locations)
        B, H, W = self._shape
        K = (2 * self.radius + 1) ** 2
        out = torch.empty((B, self.num_levels * K, H, W), dtype=torch.float32, device=self._device)
        D.corr_pyramid_lookup_device(self._ctx, self._volume, self.num_levels, self.radius, coords, out, per_level=False)
        return out


class OnDemandCorrelation:
    """``CorrelationPyramid``'s lookups without its volume (upstream RAFT's ``alternate_corr``): construction transposes the
    two float32 CUDA feature maps [B, C, H, W] and pools ``fmap1`` through ``num_levels`` levels into one workspace of
    4 * B * C * (H * W + sum_l H_l * W_l) bytes, and every lookup computes the correlation values its windows read, by the HIP kernels of
    raft_corr_ondemand_kernels.hip.  Same arguments, checks, ``num_levels`` / ``radius`` attributes, ``__call__`` and ``lookup`` results as
    ``CorrelationPyramid``; level 0 is bit-identical to it, levels >= 1 are the same quantity with other roundings.  There is no
    ``correlation_pyramid`` attribute: no correlation value is ever stored."""

    def __init__(self, fmap0, fmap1, num_levels: int, radius: int):
        import torch  # not device._torch(): a CPU tensor is refused below, as a ValueError, on a machine without a device too

        # CorrelationPyramid's checks and messages; where the tensor is comes last, so that every other complaint is also made without a device
        for name, t in (("fmap0", fmap0), ("fmap1", fmap1)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4:
                raise ValueError(f"{name} must be a 4-D float32 CUDA tensor [B, C, H, W] (no CPU fallback, no other dtype)")
        if fmap0.size() != fmap1.size() or fmap0.device != fmap1.device:
            raise ValueError(f"fmap0 and fmap1 must have the same size and device: {tuple(fmap0.shape)} on {fmap0.device} vs "
                             f"{tuple(fmap1.shape)} on {fmap1.device}")
        for name, t in (("fmap0", fmap0), ("fmap1", fmap1)):
            if not t.is_cuda:
                raise ValueError(f"{name} must be a 4-D float32 CUDA tensor [B, C, H, W] (no CPU fallback, no other dtype)")
        _check_no_grad(torch, fmap0, fmap1, what="OnDemandCorrelation")
        if not 0 <= int(radius) <= N.FTK_CORR_MAX_RADIUS:
            raise ValueError(f"radius {radius} outside 0 .. {N.FTK_CORR_MAX_RADIUS}")
        B, C, H, W = fmap0.shape
        try:
            elements, _, _ = N.corr_ondemand_layout(B, C, H, W, int(num_levels))
        except N.FtkError as e:
            raise ValueError(f"OnDemandCorrelation of {H} x {W} feature maps with num_levels={num_levels}: {e}") from None
        self.num_levels = int(num_levels)
        self.radius = int(radius)
        self._shape = (B, H, W)
        self._channels = int(C)
        self._device = fmap0.device
        self._ctx = _device_context(fmap0)
        self._workspace = torch.empty(elements, dtype=torch.float32, device=fmap0.device)
        D.corr_ondemand_prepare_device(self._ctx, fmap0.contiguous(), fmap1.contiguous(), self.num_levels, self._workspace)

    @property
    def workspace_bytes(self) -> int:
        """Bytes of the one buffer this object holds: 4 * B * C * (H * W + sum_l H_l * W_l)."""
        return 4 * int(self._workspace.numel())

    _coords = CorrelationPyramid._coords

    def __call__(self, pixel_locations):
        """As ``CorrelationPyramid.__call__``: per level a contiguous [B, H, W, (2r+1)^2] tensor of the bilinear window samples."""
        torch = D._torch()
        coords = self._coords(pixel_locations)
        B, H, W = self._shape
        K = (2 * self.radius + 1) ** 2
        block = B * H * W * K
        out = torch.empty(self.num_levels * block, dtype=torch.float32, device=self._device)
        D.corr_ondemand_lookup_device(self._ctx, self._workspace, self._channels, self.num_levels, self.radius, coords, out, per_level=True)
        return [out[l * block:(l + 1) * block].view(B, H, W, K) for l in range(self.num_levels)]

    def lookup(self, pixel_locations):
        """As ``CorrelationPyramid.lookup``: [B, L*K, H, W] in one launch."""
        torch = D._torch()
        coords = self._coords(pixel_locations)
        B, H, W = self._shape
        K = (2 * self.radius + 1) ** 2
        out = torch.empty((B, self.num_levels * K, H, W), dtype=torch.float32, device=self._device)
        D.corr_ondemand_lookup_device(self._ctx, self._workspace, self._channels, self.num_levels, self.radius, coords, out, per_level=False)
        return out


def upsample_flow(flow, mask, mask_scale: float = 1.0):
    """``Raft.UpsampleFlow(flow, mask_scale * mask)`` (model.py:48-64; update_block.py:66 is the 0.25 that ``mask_scale`` folds in):
    ``flow`` [B, 2, H, W] and ``mask`` [B, 576, H, W], float32 CUDA tensors, give a new [B, 2, 8H, 8W] tensor — per fine pixel the
    softmax of its 9 logits applied to 8 * flow of the zero-padded 3 x 3 coarse neighbourhood, by one HIP kernel
    (raft_upsample_kernels.hip) on torch's current stream.  ``B`` is just the leading dimension: the flows and masks of T iterations
    stacked as [T * B, ...] take one call.  Arguments are checked before any device is touched."""
    import torch

    for name, t, channels in (("flow", flow, 2), ("mask", mask, 576)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.size(1) != channels:
            got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{name} must be a 4-D float32 CUDA tensor [B, {channels}, H, W] (no CPU fallback, no other dtype): got {got}")
    B, _, H, W = flow.shape
    if tuple(mask.shape) != (B, 576, H, W) or flow.device != mask.device:
        raise ValueError(f"flow and mask must agree in B, H, W and device: {tuple(flow.shape)} on {flow.device} vs {tuple(mask.shape)} on "
                         f"{mask.device}")
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"flow must not be empty (got {tuple(flow.shape)})")
    if not math.isfinite(float(mask_scale)):
        raise ValueError(f"mask_scale must be finite (got {mask_scale})")
    if not flow.is_cuda:
        raise ValueError(f"flow and mask must be CUDA tensors (got them on {flow.device}): there is no CPU fallback")
    _check_no_grad(torch, flow, mask, what="upsample_flow")
    torch = D._torch()
    ctx = _device_context(flow)
    out = torch.empty((B, 2, 8 * H, 8 * W), dtype=torch.float32, device=flow.device)
    D.flow_upsample_device(ctx, flow.contiguous(), mask.contiguous(), out, mask_scale)
    return out


def _check_points(points, B: int, device) -> None:
    """``points`` of a tracking call: a float32 tensor [B, N, 2] on ``device``; where it is comes last."""
    import torch

    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() != 3 or points.size(2) != 2 or points.size(0) != B:
        got = f"{points.dtype} {list(points.shape)}" if isinstance(points, torch.Tensor) else type(points).__name__
        raise ValueError(f"points must be a float32 CUDA tensor [{B}, N, 2] of (x, y) pixels (no CPU fallback, no other dtype): got {got}")
    if points.device != device:
        raise ValueError(f"points must be on {device}, with the other tensors of the call (got them on {points.device})")


def track_points_from_flow(flow, mask, points, image_size, mask_scale: float = 1.0, backward=None, forward_backward: float = None):
    """Feature points through RAFT's coarse flow, the sparse counterpart of ``upsample_flow``: ``points`` [B, N, 2]
    (float32 CUDA, ``(x, y)`` in image pixels) are moved by the bilinear sample of ``upsample_flow(flow, mask, mask_scale)`` at each point,
    computed where the point reads it; no [B, 2, 8H, 8W] tensor is written.  ``image_size = (rows, cols)``, at most ``(8H, 8W)``, is the image
    the points live in.  Returns ``(cur_points [B, N, 2], status [B, N] uint8, fb_error2)``: ``TRACKED``, ``OUTSIDE`` (the reference or the
    tracked point is not within ``0 .. cols - 1`` x ``0 .. rows - 1``; a reference point outside comes back as it is) or ``NUMERIC_ERROR``
    (a non-finite result; the point comes back as it is).  ``backward=(flow_back, mask_back)`` with ``forward_backward=t`` pixels adds the
    forward-backward check: a tracked point is sent back through the backward pair, ``fb_error2`` [B, N] is its squared distance to where
    it started, and ``LARGE_RESIDUAL`` replaces ``TRACKED`` unless ``fb_error2 <= t * t``; without them ``fb_error2`` is ``None``.  One
    launch of raft_points_kernels.hip on torch's current stream.  Arguments are checked before any device is touched."""
    import torch

    named = [("flow", flow, 2), ("mask", mask, 576)]
    if (backward is None) != (forward_backward is None):
        raise ValueError("backward and forward_backward go together: the backward (flow, mask) pair and the threshold in pixels, or neither")
    if backward is not None:
        if not isinstance(backward, (tuple, list)) or len(backward) != 2:
            raise ValueError(f"backward must be a (flow_back, mask_back) pair (got {type(backward).__name__})")
        named += [("backward[0]", backward[0], 2), ("backward[1]", backward[1], 576)]
        if not float(forward_backward) >= 0 or not math.isfinite(float(forward_backward)):
            raise ValueError(f"forward_backward must be a finite number of pixels >= 0 (got {forward_backward})")
    for name, t, channels in named:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.size(1) != channels:
            got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{name} must be a 4-D float32 CUDA tensor [B, {channels}, H, W] (no CPU fallback, no other dtype): got {got}")
    B, _, H, W = (int(e) for e in flow.shape)
    for name, t, _ in named[1:]:
        if (t.size(0), t.size(2), t.size(3)) != (B, H, W) or t.device != flow.device:
            raise ValueError(f"flow and {name} must agree in B, H, W and device: {tuple(flow.shape)} on {flow.device} vs {tuple(t.shape)} on {t.device}")
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"flow must not be empty (got {tuple(flow.shape)})")
    _check_points(points, B, flow.device)
    try:
        rows, cols = (int(e) for e in image_size)
    except (TypeError, ValueError):
        raise ValueError(f"image_size must be (rows, cols) (got {image_size!r})") from None
    if not (1 <= rows <= 8 * H and 1 <= cols <= 8 * W):
        raise ValueError(f"image_size {rows} x {cols} must be within 1 .. {8 * H} x 1 .. {8 * W}, the grid of the flow")
    if not math.isfinite(float(mask_scale)):
        raise ValueError(f"mask_scale must be finite (got {mask_scale})")
    _check_no_grad(torch, points, *[t for _, t, _ in named], what="track_points_from_flow")
    if not flow.is_cuda:
        raise ValueError(f"flow, mask and points must be CUDA tensors (got them on {flow.device}): there is no CPU fallback")
    torch = D._torch()
    ctx = _device_context(flow)
    n = int(points.size(1))
    cur_points = torch.empty((B, n, 2), dtype=torch.float32, device=flow.device)
    status = torch.empty((B, n), dtype=torch.uint8, device=flow.device)
    fb_error2 = None if backward is None else torch.empty((B, n), dtype=torch.float32, device=flow.device)
    flow_back, mask_back = (None, None) if backward is None else (backward[0].contiguous(), backward[1].contiguous())
    D.flow_track_points_device(ctx, flow.contiguous(), mask.contiguous(), points.contiguous(), rows, cols, cur_points, status, fb_error2, mask_scale,
                               flow_back, mask_back, 0.0 if backward is None else float(forward_backward))
    return cur_points, status, fb_error2


def warm_start_flow(flow):
    """The warm start of RAFT on video: ``flow`` [B, 2, H, W] (float32 CUDA, channel 0 = x), the coarse flow of one image
    pair, pushed forward along itself as the start of the next pair, in place of upstream RAFT's ``forward_interpolate`` (scipy's
    ``griddata(method="nearest")`` on the host).  Source pixel ``(x, y)`` lands at ``(x + flow_x, y + flow_y)`` and is valid strictly
    inside ``(0, W) x (0, H)``; every pixel of the new [B, 2, H, W] tensor takes both components of the valid landing nearest to it
    (``d2 = fmaf(ey, ey, ex * ex)`` in float32, the lowest source index among equal distances); an entry without a valid landing is all
    +0.  ``H * W`` is at most ``FTK_FLOW_WARM_MAX_PIXELS`` = 2^20: the search is exhaustive.  One launch of raft_warm_kernels.hip on
    torch's current stream, or two through a workspace that torch owns when the sources are split to fill the chip; no synchronisation,
    capturable.  Arguments are checked before any device is touched."""
    import torch

    if not isinstance(flow, torch.Tensor) or flow.dtype != torch.float32 or flow.dim() != 4 or flow.size(1) != 2:
        got = f"{flow.dtype} {list(flow.shape)}" if isinstance(flow, torch.Tensor) else type(flow).__name__
        raise ValueError(f"flow must be a 4-D float32 CUDA tensor [B, 2, H, W] (no CPU fallback, no other dtype): got {got}")
    B, _, H, W = (int(e) for e in flow.shape)
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"flow must not be empty (got {tuple(flow.shape)})")
    if H * W > N.FTK_FLOW_WARM_MAX_PIXELS:
        raise ValueError(f"flow of {H} x {W} pixels is above FTK_FLOW_WARM_MAX_PIXELS = {N.FTK_FLOW_WARM_MAX_PIXELS}: the search is exhaustive")
    if not flow.is_contiguous():
        raise ValueError(f"flow must be contiguous (got strides {list(flow.stride())}): pass flow.contiguous()")
    _check_no_grad(torch, flow, what="warm_start_flow")
    if not flow.is_cuda:
        raise ValueError(f"flow must be a CUDA tensor (got it on {flow.device}): there is no CPU fallback")
    torch = D._torch()
    ctx = _device_context(flow)
    splits = N.flow_warm_splits(B, H, W)
    out = torch.empty_like(flow)
    workspace = torch.empty(splits * B * H * W, dtype=torch.int64, device=flow.device) if splits > 1 else None
    D.flow_warm_device(ctx, flow, out, splits, workspace)
    return out


class SepConvGru:
    """gru.py:46-76 (built at update_block.py:53): the separable ConvGRU, a horizontal 1 x ks pass and then a vertical ks x 1 pass, each
    z = sigmoid(conv_z([x, h])), r = sigmoid(conv_r([x, h])), q = tanh(conv_q([x, r * h])), h = (1 - z) * h + z * q.  A call is four
    launches of raft_gru_kernels.hip (per pass: the stacked z | r convolution with its sigmoids and r * h; the q convolution with tanh
    and the blend), in the arithmetic DESIGN.md 5.13 fixes.  Not an nn.Module (the package imports torch lazily): the weights live in
    ``self.weights`` under the reference's names and are packed into the kernels' layout once, by ``load`` / ``from_state_dict``."""

    GATES = ("z_horizontal", "r_horizontal", "q_horizontal", "z_vertical", "r_vertical", "q_vertical")

    def __init__(self, x_channels: int, h_channels: int, kernel_size: int = 5):
        if int(kernel_size) not in N.FTK_SEP_CONV_GRU_KERNEL_SIZES:
            raise ValueError(f"kernel_size {kernel_size} is not supported: 3 and 5 are")
        if int(x_channels) < 1 or not 1 <= int(h_channels) <= N.FTK_SEP_CONV_GRU_MAX_H_CHANNELS:
            raise ValueError(f"x_channels {x_channels} must be >= 1 and h_channels {h_channels} in 1 .. {N.FTK_SEP_CONV_GRU_MAX_H_CHANNELS}")
        if int(x_channels) + int(h_channels) > N.FTK_SEP_CONV_GRU_MAX_IN_CHANNELS:
            raise ValueError(f"x_channels + h_channels = {int(x_channels) + int(h_channels)} above {N.FTK_SEP_CONV_GRU_MAX_IN_CHANNELS}")
        self.x_channels, self.h_channels, self.kernel_size = int(x_channels), int(h_channels), int(kernel_size)
        self.weights: Dict[str, object] = {}
        self._packed: Dict[str, object] = {}

    def parameter_shapes(self) -> Dict[str, tuple]:
        """The twelve names of the reference module's state dict and their shapes."""
        C, Ch, ks = self.x_channels + self.h_channels, self.h_channels, self.kernel_size
        shapes = {}
        for g in self.GATES:
            shapes[f"conv_{g}.weight"] = (Ch, C, 1, ks) if g.endswith("horizontal") else (Ch, C, ks, 1)
            shapes[f"conv_{g}.bias"] = (Ch,)
        return shapes

    @classmethod
    def from_state_dict(cls, state: Mapping, prefix: str = "", kernel_size: int = None):
        """From a state dict of the reference's module (``Raft(...).update_block.gru.state_dict()``, or a whole model's with
        ``prefix="update_block.gru."``): the sizes are read off ``conv_z_horizontal.weight``."""
        import torch

        key = f"{prefix}conv_z_horizontal.weight"
        w = state.get(key) if hasattr(state, "get") else None
        if not isinstance(w, torch.Tensor) or w.dim() != 4 or w.size(2) != 1:
            raise ValueError(f"{key} must be a 4-D tensor [h_channels, x_channels + h_channels, 1, kernel_size]"
                             + (f" (got {list(w.shape)})" if isinstance(w, torch.Tensor) else " and is missing"))
        Ch, C, _, ks = (int(e) for e in w.shape)
        if kernel_size is not None and int(kernel_size) != ks:
            raise ValueError(f"{key} has kernel_size {ks}, not {kernel_size}")
        if C <= Ch:
            raise ValueError(f"{key} has {C} input channels for {Ch} hidden ones: x_channels must be >= 1")
        gru = cls(C - Ch, Ch, ks)
        gru.load(state, prefix)
        return gru

    def load(self, state: Mapping, prefix: str = "") -> None:
        """Takes the twelve tensors (float32, one device, the shapes of ``parameter_shapes``) and packs them; a ValueError names the key."""
        import torch

        taken, device = {}, None
        for name, shape in self.parameter_shapes().items():
            key = prefix + name
            t = state.get(key) if hasattr(state, "get") else None
            if t is None:
                raise ValueError(f"{key} is missing from the state dict")
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape:
                got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"{key} must be a float32 tensor of shape {list(shape)} (got {got})")
            device = t.device if device is None else device
            if t.device != device:
                raise ValueError(f"{key} is on {t.device}, the other weights on {device}")
            taken[name] = t.detach()
        self.weights = taken
        self._packed = self._pack(taken)

    def _pack(self, w) -> Dict[str, object]:
        """The packed matrices (``_pack_matrix`` of torch's own [M, K], k = c * ks + t) and biases, per pass.  Construction time: torch ops."""
        import torch

        K = (self.x_channels + self.h_channels) * self.kernel_size
        k_steps = N.sep_conv_gru_k_steps(self.x_channels + self.h_channels, self.kernel_size)

        packed = {}
        for d in ("horizontal", "vertical"):
            flat = {g: w[f"conv_{g}_{d}.weight"].reshape(self.h_channels, K) for g in "zrq"}
            packed["zr_" + d] = _pack_matrix(torch.cat([flat["z"], flat["r"]], 0), k_steps)
            packed["zr_bias_" + d] = torch.cat([w[f"conv_z_{d}.bias"], w[f"conv_r_{d}.bias"]], 0).contiguous()
            packed["q_" + d] = _pack_matrix(flat["q"], k_steps)
            packed["q_bias_" + d] = w[f"conv_q_{d}.bias"].contiguous()
        return packed

    def __call__(self, x, h):
        """``SepConvGru.forward(cat(x), h)``: ``x`` one float32 CUDA tensor [B, x_channels, H, W] or a sequence of up to three whose
        channels sum to x_channels (a caller passes ``(inp, out, flow)``: neither update_block.py:41's nor :63's ``cat`` is needed);
        ``h`` [B, h_channels, H, W].  Returns the new hidden state as a new tensor; nothing passed in is modified."""
        import torch

        parts = [x] if isinstance(x, torch.Tensor) else list(x) if isinstance(x, (list, tuple)) else None
        if parts is None or not 1 <= len(parts) <= N.FTK_SEP_CONV_GRU_MAX_PARTS:
            raise ValueError(f"x must be a tensor or a sequence of 1 .. {N.FTK_SEP_CONV_GRU_MAX_PARTS} tensors (got "
                             f"{type(x).__name__}{'' if parts is None else ' of ' + str(len(parts))})")
        named = [("h", h)] + [(f"x[{i}]" if len(parts) > 1 else "x", p) for i, p in enumerate(parts)]
        for name, t in named:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4:
                got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"{name} must be a 4-D float32 CUDA tensor [B, channels, H, W] (no CPU fallback, no other dtype): got {got}")
        B, Ch, H, W = h.shape
        if Ch != self.h_channels:
            raise ValueError(f"h has {Ch} channels, this SepConvGru {self.h_channels}")
        if min(B, H, W) < 1:
            raise ValueError(f"h must not be empty (got {tuple(h.shape)})")
        for name, t in named[1:]:
            if (t.size(0), t.size(2), t.size(3)) != (B, H, W) or t.size(1) < 1 or t.device != h.device:
                raise ValueError(f"{name} and h must agree in B, H, W and device: {tuple(t.shape)} on {t.device} vs {tuple(h.shape)} on {h.device}")
        if sum(int(p.size(1)) for p in parts) != self.x_channels:
            raise ValueError(f"the channels of x sum to {sum(int(p.size(1)) for p in parts)}, this SepConvGru has x_channels {self.x_channels}")
        if not self._packed:
            raise ValueError("this SepConvGru has no weights yet: load(state_dict) or SepConvGru.from_state_dict(state_dict)")
        _check_no_grad(torch, h, *parts, what="SepConvGru")
        if not h.is_cuda:
            raise ValueError(f"x and h must be CUDA tensors (got them on {h.device}): there is no CPU fallback")
        if self._packed["q_horizontal"].device != h.device:
            raise ValueError(f"the weights are on {self._packed['q_horizontal'].device}, x and h on {h.device}")
        torch = D._torch()
        ctx = _device_context(h)
        z, rh, mid, out = (torch.empty((B, Ch, H, W), dtype=torch.float32, device=h.device) for _ in range(4))
        D.sep_conv_gru_device(ctx, [p.contiguous() for p in parts], h.contiguous(), self._packed, self.kernel_size, z, rh, mid, out)
        return out


# ---- the stock layers of UpdateBlock (update_block.py:4-67) -------------------------------------------------------


def _state_tensor(state: Mapping, key: str, rank: int = None):
    """``state[key]`` as a tensor, or a ValueError that names the key."""
    import torch

    t = state.get(key) if hasattr(state, "get") else None
    if t is None:
        raise ValueError(f"{key} is missing from the state dict")
    if not isinstance(t, torch.Tensor) or (rank is not None and t.dim() != rank):
        got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{key} must be a {'' if rank is None else str(rank) + '-D '}tensor (got {got})")
    return t


def _pack_matrix(matrix, k_steps: int):
    """include/ftk.h's layout of a weight matrix [M, K] in torch's own k order: padded to whole tiles and k-steps (rows +0, columns -0), as
    [tiles][k_steps][64] with lane = 32 (k % 2) + row % 32.  Construction time: torch ops."""
    import torch

    M, K = (int(e) for e in matrix.shape)
    tiles = -(-M // 32)
    full = torch.zeros((tiles * 32, 2 * k_steps), dtype=torch.float32, device=matrix.device)
    full[:, K:] = -0.0
    full[:M, :K] = matrix
    return full.view(tiles, 32, k_steps, 2).permute(0, 2, 3, 1).contiguous().view(-1)


def _pack_conv(weight):
    """The packed matrix of a Conv2d weight [M, C_in, ks, ks]: ``_pack_matrix`` of torch's own [M, K], k = (c * ks + ty) * ks + tx."""
    M, Cin, ks, _ = (int(e) for e in weight.shape)
    return _pack_matrix(weight.reshape(M, Cin * ks * ks), N.conv2d_k_steps(Cin, ks))


def _load_convs(state: Mapping, prefix: str, shapes: Mapping):
    """The Conv2d layers ``shapes`` names (layer -> (out_channels, in_channels, kernel_size)) from ``state``: float32, one device, those
    shapes.  Returns the tensors under the reference's names and, per layer, (packed weights, bias, kernel_size, out_channels)."""
    import torch

    taken, packed, device = {}, {}, None
    for layer, (M, Cin, ks) in shapes.items():
        if ks not in N.FTK_CONV2D_KERNEL_SIZES or not 1 <= M <= N.FTK_CONV2D_MAX_OUT_CHANNELS or not 1 <= Cin <= N.FTK_CONV2D_MAX_IN_CHANNELS:
            raise ValueError(f"{prefix}{layer}.weight: a {ks} x {ks} convolution of {Cin} -> {M} channels is outside the supported sizes (kernel size "
                             f"1, 3 or 7, up to {N.FTK_CONV2D_MAX_IN_CHANNELS} -> {N.FTK_CONV2D_MAX_OUT_CHANNELS} channels)")
        for kind, shape in (("weight", (M, Cin, ks, ks)), ("bias", (M,))):
            key = f"{prefix}{layer}.{kind}"
            t = _state_tensor(state, key)
            if t.dtype != torch.float32 or tuple(t.shape) != shape:
                raise ValueError(f"{key} must be a float32 tensor of shape {list(shape)} (got {t.dtype} {list(t.shape)})")
            device = t.device if device is None else device
            if t.device != device:
                raise ValueError(f"{key} is on {t.device}, the other weights on {device}")
            taken[f"{layer}.{kind}"] = t.detach()
        packed[layer] = (_pack_conv(taken[f"{layer}.weight"]), taken[f"{layer}.bias"].contiguous(), ks, M)
    return taken, packed


def _check_maps(what: str, named, weights_device) -> tuple:
    """The feature maps of a call, ``named`` = [(name, tensor, channels)]: 4-D float32 tensors of those channel counts that agree in B, H, W
    and device, not empty, not requiring grad, on the device of the weights, which is a CUDA device.  Returns (B, H, W)."""
    import torch

    for name, t, channels in named:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.size(1) != channels:
            got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{name} must be a 4-D float32 CUDA tensor [B, {channels}, H, W] (no CPU fallback, no other dtype): got {got}")
    first_name, first, _ = named[0]
    B, _, H, W = first.shape
    for name, t, _ in named[1:]:
        if (t.size(0), t.size(2), t.size(3)) != (B, H, W) or t.device != first.device:
            raise ValueError(f"{name} and {first_name} must agree in B, H, W and device: {tuple(t.shape)} on {t.device} vs {tuple(first.shape)} on "
                             f"{first.device}")
    if min(B, H, W) < 1:
        raise ValueError(f"{first_name} must not be empty (got {tuple(first.shape)})")
    if weights_device is None:
        raise ValueError(f"this {what} has no weights yet: load(state_dict) or {what}.from_state_dict(state_dict)")
    _check_no_grad(torch, *[t for _, t, _ in named], what=what)
    if not first.is_cuda:
        raise ValueError(f"the inputs must be CUDA tensors (got them on {first.device}): there is no CPU fallback")
    if weights_device != first.device:
        raise ValueError(f"the weights are on {weights_device}, the inputs on {first.device}")
    return int(B), int(H), int(W)


def _conv(ctx, parts, layer, relu: bool, out_scale: float = 1.0):
    """One launch of conv2d_kernel over checked, contiguous ``parts``; ``layer`` as _load_convs makes it.  Returns a new tensor."""
    torch = D._torch()
    weights, bias, ks, M = layer
    B, _, H, W = parts[0].shape
    out = torch.empty((B, M, H, W), dtype=torch.float32, device=parts[0].device)
    D.conv2d_device(ctx, parts, weights, bias, ks, relu, out_scale, out)
    return out




class MotionEncoder:
    """update_block.py:16-43: ``correlation_conv`` (1 x 1, ReLU, 3 x 3, ReLU) on the correlation features, ``flow_conv`` (7 x 7, ReLU, 3 x 3,
    ReLU) on the flow, ``out_conv`` (3 x 3, ReLU) on their concatenation, which is read in place as two parts and never stored.  Five
    launches of raft_conv_kernels.hip in the arithmetic DESIGN.md 5.14 fixes.  Not an nn.Module (the package imports torch lazily): the
    weights live in ``self.weights`` under the reference's names and are packed into the kernels' layout once, by ``load`` /
    ``from_state_dict``."""

    def __init__(self, correlation_in: int, correlation_hidden: int, correlation_out: int, flow_hidden: int, flow_out: int, out_channels: int):
        sizes = dict(correlation_in=correlation_in, correlation_hidden=correlation_hidden, correlation_out=correlation_out, flow_hidden=flow_hidden,
                     flow_out=flow_out, out_channels=out_channels)
        for name, v in sizes.items():
            if int(v) < (3 if name == "out_channels" else 1):
                raise ValueError(f"{name} {v} must be at least {3 if name == 'out_channels' else 1}")
        self.correlation_in, self.correlation_hidden, self.correlation_out = int(correlation_in), int(correlation_hidden), int(correlation_out)
        self.flow_hidden, self.flow_out, self.out_channels = int(flow_hidden), int(flow_out), int(out_channels)
        for layer, (M, Cin, ks) in self.layer_shapes().items():
            if M > N.FTK_CONV2D_MAX_OUT_CHANNELS or Cin > N.FTK_CONV2D_MAX_IN_CHANNELS:
                raise ValueError(f"{layer}: {Cin} -> {M} channels above {N.FTK_CONV2D_MAX_IN_CHANNELS} -> {N.FTK_CONV2D_MAX_OUT_CHANNELS}")
        self.weights: Dict[str, object] = {}
        self._layers: Dict[str, tuple] = {}

    def layer_shapes(self) -> Dict[str, tuple]:
        """The five Conv2d layers under the reference's names: (out_channels, in_channels, kernel_size)."""
        return {"correlation_conv.0": (self.correlation_hidden, self.correlation_in, 1),
                "correlation_conv.2": (self.correlation_out, self.correlation_hidden, 3),
                "flow_conv.0": (self.flow_hidden, 2, 7),
                "flow_conv.2": (self.flow_out, self.flow_hidden, 3),
                "out_conv.0": (self.out_channels - 2, self.correlation_out + self.flow_out, 3)}

    @classmethod
    def from_state_dict(cls, state: Mapping, prefix: str = ""):
        """From a state dict of the reference's module (``Raft(...).update_block.motion_encoder.state_dict()``, or a whole model's with
        ``prefix="update_block.motion_encoder."``): the sizes are read off the weights."""
        w = {layer: _state_tensor(state, f"{prefix}{layer}.weight", 4) for layer in ("correlation_conv.0", "correlation_conv.2", "flow_conv.0", "flow_conv.2",
                                                                                      "out_conv.0")}
        enc = cls(w["correlation_conv.0"].size(1), w["correlation_conv.0"].size(0), w["correlation_conv.2"].size(0), w["flow_conv.0"].size(0),
                  w["flow_conv.2"].size(0), w["out_conv.0"].size(0) + 2)
        enc.load(state, prefix)
        return enc

    def load(self, state: Mapping, prefix: str = "") -> None:
        """Takes the ten tensors (float32, one device, the shapes of ``layer_shapes``) and packs them; a ValueError names the key."""
        self.weights, self._layers = _load_convs(state, prefix, self.layer_shapes())

    def _weights_device(self):
        return self._layers["out_conv.0"][0].device if self._layers else None

    def _features(self, ctx, correlation, flow):
        L = self._layers
        temp_correlation = _conv(ctx, [_conv(ctx, [correlation], L["correlation_conv.0"], True)], L["correlation_conv.2"], True)
        temp_flow = _conv(ctx, [_conv(ctx, [flow], L["flow_conv.0"], True)], L["flow_conv.2"], True)
        return _conv(ctx, [temp_correlation, temp_flow], L["out_conv.0"], True)

    def features(self, correlation, flow):
        """update_block.py:37-40: ``out_conv(cat[correlation_conv(correlation), flow_conv(flow)])`` as a new [B, out_channels - 2, H, W]
        tensor, in five launches on torch's current stream; ``correlation`` [B, correlation_in, H, W] and ``flow`` [B, 2, H, W] are float32
        CUDA tensors.  Nothing passed in is modified."""
        _check_maps("MotionEncoder", [("correlation", correlation, self.correlation_in), ("flow", flow, 2)], self._weights_device())
        return self._features(_device_context(flow), correlation.contiguous(), flow.contiguous())

    def __call__(self, correlation, flow):
        """``MotionEncoder.forward`` (update_block.py:36-43): ``cat([features(correlation, flow), flow])``, [B, out_channels, H, W].  The cat is
        torch's, and the only one; a caller that feeds SepConvGru passes ``(inp, features, flow)`` as parts instead and needs none."""
        import torch

        return torch.cat([self.features(correlation, flow), flow], dim=1)


class UpdateBlock:
    """update_block.py:45-67: one refinement iteration of RAFT, ``(net, inp, correlation, flow) -> (new_net, mask, delta_flow)``: the motion
    encoder (5 launches), ``SepConvGru((inp, out, flow), net)`` (4), the flow head (2) and the mask head (2) whose last layer carries
    :66's 0.25: 13 launches on torch's current stream, no ``cat`` and no element-wise pass.  Built from a state
    dict of the reference's module; not an nn.Module.  ``self.weights`` holds every tensor under the reference's names."""

    def __init__(self, motion_encoder: MotionEncoder, gru: SepConvGru, state: Mapping, prefix: str):
        net = gru.h_channels
        self.net_channels, self.inp_channels = net, gru.x_channels - motion_encoder.out_channels
        self.motion_encoder, self.gru = motion_encoder, gru
        hidden = _state_tensor(state, f"{prefix}flow_head.conv1.weight", 4).size(0)
        mask_hidden = _state_tensor(state, f"{prefix}mask.0.weight", 4).size(0)
        mask_out = _state_tensor(state, f"{prefix}mask.2.weight", 4).size(0)
        self.mask_hidden_channels, self.mask_channels = int(mask_hidden), int(mask_out)
        heads, self._layers = _load_convs(state, prefix, {"flow_head.conv1": (int(hidden), net, 3), "flow_head.conv2": (2, int(hidden), 3),
                                                          "mask.0": (int(mask_hidden), net, 3), "mask.2": (int(mask_out), int(mask_hidden), 1)})
        self.weights: Dict[str, object] = {"motion_encoder." + k: v for k, v in motion_encoder.weights.items()}
        self.weights.update({"gru." + k: v for k, v in gru.weights.items()})
        self.weights.update(heads)

    @classmethod
    def from_state_dict(cls, state: Mapping, prefix: str = "update_block."):
        """From a state dict of the reference's ``Raft`` (the default prefix) or of its ``UpdateBlock`` alone (``prefix=""``).  All sizes are
        read off the weights; a missing or mis-shaped tensor is a ValueError that names its key."""
        encoder = MotionEncoder.from_state_dict(state, prefix + "motion_encoder.")
        gru = SepConvGru.from_state_dict(state, prefix + "gru.")
        if gru.x_channels <= encoder.out_channels:
            raise ValueError(f"{prefix}gru.conv_z_horizontal.weight has {gru.x_channels} channels of x: fewer than inp (at least 1) and the motion "
                             f"encoder's {encoder.out_channels}")
        block = cls(encoder, gru, state, prefix)
        devices = {str(t.device) for t in block.weights.values()}
        if len(devices) != 1:
            raise ValueError(f"the weights under {prefix!r} are on several devices: {sorted(devices)}")
        return block

    def __call__(self, net, inp, correlation, flow, want_mask: bool = True):
        """``UpdateBlock.forward``: float32 CUDA tensors ``net`` [B, net, H, W], ``inp`` [B, inp, H, W], ``correlation`` [B, corr, H, W] and
        ``flow`` [B, 2, H, W] give new tensors ``(new_net, mask, delta_flow)``; ``mask`` already carries the 0.25.  Every argument is
        checked before the first launch; nothing passed in is modified.  ``want_mask=False`` skips the mask head's two launches and returns
        ``None`` for ``mask`` (a caller that uses only the last iteration's mask, ``Raft.track_points``); the other two results do not
        depend on it."""
        enc = self.motion_encoder
        _check_maps("UpdateBlock", [("net", net, self.net_channels), ("inp", inp, self.inp_channels), ("correlation", correlation, enc.correlation_in),
                                    ("flow", flow, 2)], enc._weights_device())
        ctx = _device_context(net)
        flow = flow.contiguous()
        out = enc._features(ctx, correlation.contiguous(), flow)
        new_net = self.gru((inp, out, flow), net)
        L = self._layers
        delta_flow = _conv(ctx, [_conv(ctx, [new_net], L["flow_head.conv1"], True)], L["flow_head.conv2"], False)
        mask = _conv(ctx, [_conv(ctx, [new_net], L["mask.0"], True)], L["mask.2"], False, 0.25) if want_mask else None
        return new_net, mask, delta_flow


# ---- the encoders and the whole model (encoder.py:4-68, model.py:6-97) --------------------------------------------

BN_EPS = 1e-5  # nn.BatchNorm2d's default; the module stores none
CORRELATION_MODES = ("all_pairs", "on_demand")  # Raft(correlation=...): CorrelationPyramid (the reference's) or OnDemandCorrelation


def _fold_batch_norm(state: Mapping, conv_key: str, bn_prefix: str, eps: float):
    """``conv`` (no bias) followed by ``BatchNorm2d`` in eval mode as one layer: s = gamma / sqrt(var + eps), w' = w * s, b' = beta - mean * s,
    on the host in numpy float32, every operation rounded once.  ``num_batches_tracked`` is read and ignored.  Returns
    (w', b') on the weights' device."""
    import numpy as np
    import torch

    w = _state_tensor(state, conv_key, 4)
    if w.dtype != torch.float32:
        raise ValueError(f"{conv_key} must be a float32 tensor (got {w.dtype} {list(w.shape)})")
    M = int(w.size(0))
    bn = {}
    for kind in ("weight", "bias", "running_mean", "running_var"):
        key = bn_prefix + kind
        t = _state_tensor(state, key)
        if t.dtype != torch.float32 or tuple(t.shape) != (M,):
            raise ValueError(f"{key} must be a float32 tensor of shape {[M]} (got {t.dtype} {list(t.shape)})")
        if t.device != w.device:
            raise ValueError(f"{key} is on {t.device}, the other weights on {w.device}")
        bn[kind] = t.detach().cpu().numpy()
    _state_tensor(state, bn_prefix + "num_batches_tracked")
    # numpy, not torch: its float32 division and square root are the correctly rounded scalar ones on every CPU, which torch's vectorised
    # sqrt is not on every host (it has differed from sqrtf in the last bit)
    with np.errstate(all="ignore"):
        shifted = bn["running_var"] + np.float32(eps)
        if not bool((shifted > 0).all()):
            raise ValueError(f"{bn_prefix}running_var + eps must be positive (smallest: {float(shifted.min())})")
        scale = bn["weight"] / np.sqrt(shifted)
        if not bool(np.isfinite(scale).all()):
            raise ValueError(f"{bn_prefix}weight / sqrt({bn_prefix}running_var + eps) is not finite")
        folded_w = torch.from_numpy(w.detach().cpu().numpy() * scale.reshape(M, 1, 1, 1))
        folded_b = torch.from_numpy(bn["bias"] - bn["running_mean"] * scale)
    return folded_w.to(w.device), folded_b.to(w.device)


def _strided_conv(ctx, x, layer, stride: int, relu: bool, residual=None, normalise: bool = False):
    """One launch over a checked, contiguous ``x``; ``layer`` = (packed weights, bias, kernel_size, out_channels).  Returns a new tensor."""
    torch = D._torch()
    weights, bias, ks, M = layer
    B, _, H, W = x.shape
    out = torch.empty((B, M, -(-H // stride), -(-W // stride)), dtype=torch.float32, device=x.device)
    D.conv2d_strided_device(ctx, [x], weights, bias, ks, stride, relu, 1.0, residual, normalise, out)
    return out


class FeatureEncoder:
    """encoder.py:25-55: ``conv_in`` (7 x 7, bias, ReLU), three pairs of ``ResNetBlock`` (the second of each pair at stride 2 with a
    projecting 1 x 1 shortcut) and ``conv_out`` (3 x 3, bias, ReLU): [B, in_channels, H, W] -> [B, out_channels, ~H/8, ~W/8] in 17 launches
    of raft_conv_kernels.hip.  Every BatchNorm is folded into its convolution once, at construction; a block is ``relu(conv1')``, the
    shortcut (``x`` itself, or ``shortcut'(x)``) and ``relu(conv2'(t) + shortcut)`` with the add in conv2's epilogue.  ``normalise=True``
    applies model.py:70-71 to the image as conv_in fetches it.  Not an nn.Module; ``self.weights`` holds the state dict's tensors under the
    reference's names."""

    BLOCKS = tuple((f"resnet_{k}.{i}", 1 + i) for k in (1, 2, 3) for i in (0, 1))  # (name, stride): encoder.py:33-44

    def __init__(self, state: Mapping, prefix: str = "", eps: float = BN_EPS, _split=None):
        import torch

        self.eps = float(eps)
        if not 0 <= self.eps < float("inf"):
            raise ValueError(f"eps must be a finite non-negative number (got {eps})")
        names = set(state.keys()) if hasattr(state, "keys") else set()
        taken: Dict[str, object] = {}
        convs: Dict[str, tuple] = {}  # layer -> (w', b')

        def take(key):
            taken[key[len(prefix):]] = _state_tensor(state, key).detach()

        def plain(layer, ks):
            w = _state_tensor(state, f"{prefix}{layer}.weight", 4)
            M, Cin = int(w.size(0)), int(w.size(1))
            for kind, shape in (("weight", (M, Cin, ks, ks)), ("bias", (M,))):
                key = f"{prefix}{layer}.{kind}"
                t = _state_tensor(state, key)
                if t.dtype != torch.float32 or tuple(t.shape) != shape:
                    raise ValueError(f"{key} must be a float32 tensor of shape {list(shape)} (got {t.dtype} {list(t.shape)})")
                take(key)
            convs[layer] = (taken[f"{layer}.weight"], taken[f"{layer}.bias"])
            return M, Cin

        def folded(conv, bn, ks, Cin, M=None):
            w = _state_tensor(state, f"{prefix}{conv}.weight", 4)
            M = int(w.size(0)) if M is None else M
            if tuple(w.shape) != (M, Cin, ks, ks):
                raise ValueError(f"{prefix}{conv}.weight must be a float32 tensor of shape {[M, Cin, ks, ks]} (got {w.dtype} {list(w.shape)})")
            convs[conv] = _fold_batch_norm(state, f"{prefix}{conv}.weight", f"{prefix}{bn}.", self.eps)
            take(f"{prefix}{conv}.weight")
            for kind in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
                take(f"{prefix}{bn}.{kind}")
            return M

        width, self.in_channels = plain("conv_in.0", 7)
        self.blocks = []  # (name, stride, has a shortcut)
        for name, stride in self.BLOCKS:
            M = folded(f"{name}.conv1", f"{name}.bn1", 3, width)
            folded(f"{name}.conv2", f"{name}.bn2", 3, M, M)
            shortcut = any(k.startswith(f"{prefix}{name}.shortcut.") for k in names) or stride != 1 or M != width
            if shortcut:
                folded(f"{name}.shortcut.0", f"{name}.shortcut.1", 1, width, M)
            self.blocks.append((name, stride, shortcut))
            width = M
        self.out_channels, last_in = plain("conv_out.0", 3)
        if last_in != width:
            raise ValueError(f"{prefix}conv_out.0.weight must be a float32 tensor of shape {[self.out_channels, width, 3, 3]} (got "
                             f"{list(taken['conv_out.0.weight'].shape)})")
        devices = {str(t.device) for t in taken.values() if t.dtype == torch.float32}
        if len(devices) != 1:
            raise ValueError(f"the weights under {prefix!r} are on several devices: {sorted(devices)}")
        for layer, (w, b) in convs.items():
            M, Cin, ks = int(w.size(0)), int(w.size(1)), int(w.size(2))
            if not 1 <= M <= N.FTK_CONV2D_MAX_OUT_CHANNELS or not 1 <= Cin <= N.FTK_CONV2D_MAX_IN_CHANNELS:
                raise ValueError(f"{prefix}{layer}.weight: {Cin} -> {M} channels is outside 1 .. {N.FTK_CONV2D_MAX_IN_CHANNELS} -> 1 .. "
                                 f"{N.FTK_CONV2D_MAX_OUT_CHANNELS}")
        self.weights = taken
        self.folded = convs
        self._split = None
        self._layers = {layer: (_pack_conv(w), b.contiguous(), int(w.size(2)), int(w.size(0))) for layer, (w, b) in convs.items()}
        if _split is not None:  # ContextEncoder: conv_out as two launches over the two row ranges of its weight matrix
            w, b = convs["conv_out.0"]
            if not 0 < _split < self.out_channels:
                raise ValueError(f"context_channels {_split} must be in 1 .. {self.out_channels - 1}: {prefix}conv_out.0.weight has {self.out_channels} "
                                 "output channels for context and hidden together")
            self._split = int(_split)
            del self._layers["conv_out.0"]
            self._layers["conv_out.0[context]"] = (_pack_conv(w[:_split]), b[:_split].contiguous(), 3, int(_split))
            self._layers["conv_out.0[hidden]"] = (_pack_conv(w[_split:]), b[_split:].contiguous(), 3, self.out_channels - int(_split))

    @classmethod
    def from_state_dict(cls, state: Mapping, prefix: str = "", eps: float = BN_EPS):
        """From a state dict of the reference's module, or a whole ``Raft``'s with ``prefix="feature_encoder."``.  All sizes are read off the
        weights and whether a block has a shortcut off the keys; a missing, misshapen or mistyped tensor is a ValueError that names its key."""
        return cls(state, prefix, eps)

    def _weights_device(self):
        return next(iter(self._layers.values()))[0].device

    def _trunk(self, ctx, image, normalise: bool):
        L = self._layers
        x = _strided_conv(ctx, image, L["conv_in.0"], 1, True, normalise=normalise)
        for name, stride, shortcut in self.blocks:
            t = _strided_conv(ctx, x, L[f"{name}.conv1"], stride, True)
            r = _strided_conv(ctx, x, L[f"{name}.shortcut.0"], stride, False) if shortcut else x
            x = _strided_conv(ctx, t, L[f"{name}.conv2"], 1, True, residual=r)
        return x

    def _check(self, what, image):
        _check_maps(what, [("image", image, self.in_channels)], self._weights_device())
        return _device_context(image), image.contiguous()

    def __call__(self, image, normalise: bool = False):
        """``FeatureEncoder.forward``: a float32 CUDA tensor [B, in_channels, H, W] gives a new [B, out_channels, h, w] tensor, h = H halved
        three times, each time rounded up.  Checked before the first launch; nothing passed in is modified."""
        ctx, image = self._check("FeatureEncoder", image)
        return _strided_conv(ctx, self._trunk(ctx, image, normalise), self._layers["conv_out.0"], 1, True)


class ContextEncoder:
    """encoder.py:57-68: a FeatureEncoder of ``context_channels + hidden_channels`` output channels whose result is split into ``(context,
    hidden)`` = model.py:80's ``(inp, net)``.  Both come out dense with no copy pass: conv_out runs as two launches over the two row ranges
    of its weight matrix (output channels are independent: bit-identical to the split), 18 launches in all.  The module's weights hold only
    the sum of the two widths, so ``context_channels`` is an argument."""

    def __init__(self, state: Mapping, prefix: str = "", context_channels: int = None, eps: float = BN_EPS):
        if context_channels is None or int(context_channels) < 1:
            raise ValueError(f"context_channels must be given and positive (got {context_channels}): the weights hold only context + hidden")
        self.net = FeatureEncoder(state, prefix + "net.", eps, _split=int(context_channels))
        self.context_channels = int(context_channels)
        self.hidden_channels = self.net.out_channels - self.context_channels
        self.weights = {"net." + k: v for k, v in self.net.weights.items()}

    @classmethod
    def from_state_dict(cls, state: Mapping, prefix: str = "", context_channels: int = None, eps: float = BN_EPS):
        """From a state dict of the reference's module, or a whole ``Raft``'s with ``prefix="context_encoder."``."""
        return cls(state, prefix, context_channels, eps)

    def __call__(self, image, normalise: bool = False):
        """``ContextEncoder.forward``: ``(context, hidden)``, new contiguous tensors [B, context_channels, h, w] and [B, hidden_channels, h, w]."""
        ctx, image = self.net._check("ContextEncoder", image)
        x = self.net._trunk(ctx, image, normalise)
        L = self.net._layers
        return _strided_conv(ctx, x, L["conv_out.0[context]"], 1, True), _strided_conv(ctx, x, L["conv_out.0[hidden]"], 1, True)


class Raft:
    """model.py:6-97: ``raft(ref_image, cur_image)`` returns the reference's list of flow predictions [B, 2, 8h, 8w], one per iteration.
    The feature encoder runs once over the two images stacked along B (17 launches), the context encoder on the reference image (18), both
    normalising the raw image at conv_in's fetch, and the correlation pyramid is built (1 launch up to four levels); then per iteration one lookup, UpdateBlock's 13 launches and one upsampling launch.
    What stays torch: the stack of the two raw images, the meshgrid, and the three [B, 2, h, w] element-wise operations of model.py:90-94,
    kept as written (``(cur + delta) - ref`` is not ``flow + delta`` in float32).  ``correlation="on_demand"`` replaces the pyramid by
    ``OnDemandCorrelation`` (no volume; 1 + (levels - 1) launches to prepare); the default ``"all_pairs"`` is the reference's."""

    def __init__(self, feature_encoder: FeatureEncoder, context_encoder: ContextEncoder, update_block: UpdateBlock, correlation_pyramid_levels: int,
                 correlation_radius: int, max_iterations: int = 12, correlation: str = "all_pairs"):
        if correlation not in CORRELATION_MODES:
            raise ValueError(f"correlation {correlation!r} is not one of {', '.join(repr(m) for m in CORRELATION_MODES)}")
        self.correlation = correlation
        levels, radius = int(correlation_pyramid_levels), int(correlation_radius)
        if not 1 <= levels <= N.FTK_CORR_MAX_LEVELS or not 0 <= radius <= N.FTK_CORR_MAX_RADIUS:
            raise ValueError(f"correlation_pyramid_levels {correlation_pyramid_levels} outside 1 .. {N.FTK_CORR_MAX_LEVELS} or correlation_radius "
                             f"{correlation_radius} outside 0 .. {N.FTK_CORR_MAX_RADIUS}")
        width = levels * (2 * radius + 1) ** 2
        if update_block.motion_encoder.correlation_in != width:
            raise ValueError(f"the update block takes {update_block.motion_encoder.correlation_in} correlation channels, but {levels} levels of radius "
                             f"{radius} give levels * (2 * radius + 1) ** 2 = {width}")
        if int(max_iterations) < 1:
            raise ValueError(f"max_iterations {max_iterations} must be at least 1")
        if update_block.mask_channels != 576:
            raise ValueError(f"the update block's mask has {update_block.mask_channels} channels: the upsampling takes 8 * 8 * 9 = 576")
        if (context_encoder.context_channels, context_encoder.hidden_channels) != (update_block.inp_channels, update_block.net_channels):
            raise ValueError(f"the context encoder gives {context_encoder.context_channels} + {context_encoder.hidden_channels} channels, the update "
                             f"block takes inp {update_block.inp_channels} + net {update_block.net_channels}")
        if feature_encoder.in_channels != context_encoder.net.in_channels:
            raise ValueError(f"the feature encoder takes {feature_encoder.in_channels} image channels, the context encoder {context_encoder.net.in_channels}")
        self.feature_encoder, self.context_encoder, self.update_block = feature_encoder, context_encoder, update_block
        self.correlation_pyramid_levels, self.correlation_radius, self.max_iterations = levels, radius, int(max_iterations)
        self.hidden_dim, self.context_dim = update_block.net_channels, update_block.inp_channels
        self.weights: Dict[str, object] = {"feature_encoder." + k: v for k, v in feature_encoder.weights.items()}
        self.weights.update({"context_encoder." + k: v for k, v in context_encoder.weights.items()})
        self.weights.update({"update_block." + k: v for k, v in update_block.weights.items()})

    @classmethod
    def from_state_dict(cls, state: Mapping, correlation_pyramid_levels: int, correlation_radius: int, max_iterations: int = 12, eps: float = BN_EPS,
                        correlation: str = "all_pairs"):
        """From ``Raft(...).state_dict()`` of the reference.  All widths are read off the weights; the context encoder's split is the update
        block's ``inp`` and ``net`` widths.  The two correlation arguments are not in the state dict: they must give the update block's
        correlation width, levels * (2 * radius + 1) ** 2."""
        if correlation not in CORRELATION_MODES:
            raise ValueError(f"correlation {correlation!r} is not one of {', '.join(repr(m) for m in CORRELATION_MODES)}")
        block = UpdateBlock.from_state_dict(state, "update_block.")
        features = FeatureEncoder.from_state_dict(state, "feature_encoder.", eps)
        out = _state_tensor(state, "context_encoder.net.conv_out.0.weight", 4)
        if int(out.size(0)) != block.inp_channels + block.net_channels:
            raise ValueError(f"context_encoder.net.conv_out.0.weight has {int(out.size(0))} output channels, the update block takes inp "
                             f"{block.inp_channels} + net {block.net_channels}")
        context = ContextEncoder.from_state_dict(state, "context_encoder.", block.inp_channels, eps)
        devices = {str(features._weights_device()), str(context.net._weights_device()), str(block.motion_encoder._weights_device())}
        if len(devices) != 1:
            raise ValueError(f"the weights are on several devices: {sorted(devices)}")
        return cls(features, context, block, correlation_pyramid_levels, correlation_radius, max_iterations, correlation)

    @staticmethod
    def _check_flow_init(flow_init, pair: bool, B: int, h: int, w: int, device) -> None:
        """``flow_init`` of a call: None, a float32 tensor [B, 2, h, w] on ``device``, the images', or, with the forward-backward check
        (``pair``), a (forward, backward) pair of them."""
        import torch

        if flow_init is None:
            return
        if pair and (not isinstance(flow_init, (tuple, list)) or len(flow_init) != 2):
            raise ValueError(f"flow_init must be a (forward_init, backward_init) pair with forward_backward (got {type(flow_init).__name__})")
        named = [("flow_init[0]", flow_init[0]), ("flow_init[1]", flow_init[1])] if pair else [("flow_init", flow_init)]
        for name, t in named:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (B, 2, h, w):
                got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"{name} must be a float32 CUDA tensor [{B}, 2, {h}, {w}], the coarse flow of these images (no CPU fallback, no other "
                                 f"dtype): got {got}")
            if t.device != device:
                raise ValueError(f"{name} must be on {device}, with the images (got it on {t.device})")
        _check_no_grad(torch, *[t for _, t in named], what="Raft")

    def _refine(self, fmap0, fmap1, inp, net, n: int, flow_init=None, want_mask: str = "every"):
        """model.py:82-95, the refinement loop on its own: the correlation object of the feature maps ``fmap0`` and ``fmap1`` [B', C, h, w],
        ``n`` iterations from ``cur = ref`` or, with ``flow_init`` [B', 2, h, w], from ``cur = ref + flow_init`` (upstream's ``coords1 =
        coords1 + flow_init``), with ``inp`` and ``net`` of the context encoder.  ``want_mask``: "every" runs the mask head and
        ``upsample_flow`` in every iteration (``__call__``), "last" the mask head in the last iteration alone (``track_points``), "never"
        not at all.  Returns (the last ``cur - ref``, the last mask or None, the predictions of "every").  Everything was checked by the
        caller."""
        import torch

        correlation_class = OnDemandCorrelation if self.correlation == "on_demand" else CorrelationPyramid
        pyramid = correlation_class(fmap0, fmap1, self.correlation_pyramid_levels, self.correlation_radius)
        batch, _, h, w = fmap0.shape
        ys, xs = torch.meshgrid(torch.arange(h, device=fmap0.device), torch.arange(w, device=fmap0.device), indexing="ij")
        ref = torch.stack([xs, ys], dim=0).float()[None].repeat(batch, 1, 1, 1)  # InitializeFlow, model.py:34-45: x in channel 0
        cur = ref if flow_init is None else ref + flow_init
        predictions, mask, flow = [], None, None
        for i in range(n):
            correlation = pyramid.lookup(cur)
            flow = cur - ref
            net, mask, delta = self.update_block(net, inp, correlation, flow, want_mask=want_mask == "every" or (want_mask == "last" and i == n - 1))
            cur = cur + delta
            if want_mask == "every":
                flow = cur - ref
                predictions.append(upsample_flow(flow, mask))
        if want_mask != "every":
            flow = cur - ref
        return flow, mask, predictions

    def __call__(self, ref_image, cur_image, iterations: int = None, flow_init=None, return_flow: bool = False):
        """``Raft.forward``: float32 CUDA images [B, in_channels, H, W] in 0 .. 255 give ``iterations`` (default ``max_iterations``) new
        tensors [B, 2, 8h, 8w], h = H halved three times rounding up (a 60 x 60 image gives 64 x 64; nothing is cropped).  ``flow_init``
        [B, 2, h, w] (float32, the images' device) starts the loop from ``ref + flow_init`` instead of ``ref``, as upstream's
        ``flow_init`` does; ``return_flow=True`` returns ``(predictions, flow)`` with the last iteration's coarse ``cur - ref`` [B, 2, h, w],
        what ``warm_start_flow`` takes.  Every argument is checked before the first launch; on torch's current stream, capturable at fixed
        shapes."""
        import torch

        n, B, H, W, h, w = self._check_pair(ref_image, cur_image, None, iterations, False, flow_init)
        features = self.feature_encoder(torch.cat([ref_image, cur_image], dim=0), normalise=True)
        inp, net = self.context_encoder(ref_image, normalise=True)
        flow, _, predictions = self._refine(features[:B], features[B:], inp, net, n, flow_init, "every")
        return (predictions, flow) if return_flow else predictions

    def _check_pair(self, ref_image, cur_image, points, iterations, stacked: bool, flow_init=None):
        """The argument checks of a call on an image pair, with those of ``points`` (None: the call takes none) and of ``flow_init`` placed
        before the complaint about where the tensors are, so that each is also made on a machine without a device; ``stacked``: the loop
        will run at batch 2B and ``flow_init`` is a pair.  Returns (n, B, H, W, h, w)."""
        import torch

        n = self.max_iterations if iterations is None else int(iterations)
        if n < 1:
            raise ValueError(f"iterations {iterations} must be at least 1")
        enc = self.feature_encoder
        for name, t in (("ref_image", ref_image), ("cur_image", cur_image)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.size(1) != enc.in_channels:
                got = f"{t.dtype} {list(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"{name} must be a 4-D float32 CUDA tensor [B, {enc.in_channels}, H, W] (no CPU fallback, no other dtype): got {got}")
        if ref_image.size() != cur_image.size() or ref_image.device != cur_image.device:
            raise ValueError(f"The size of the reference and current images should be the same: {tuple(ref_image.shape)} on {ref_image.device} vs "
                             f"{tuple(cur_image.shape)} on {cur_image.device}")
        B, _, H, W = (int(e) for e in ref_image.shape)
        if points is not None:
            _check_points(points, B, ref_image.device)
            _check_no_grad(torch, points, what="Raft")
        h, w = ((((e + 1) // 2 + 1) // 2 + 1) // 2 for e in (H, W))  # three stride-2 layers, each ceil(e / 2)
        self._check_flow_init(flow_init, stacked, B, h, w, ref_image.device)
        _check_maps("Raft", [("ref_image", ref_image, enc.in_channels), ("cur_image", cur_image, enc.in_channels)], enc._weights_device())
        try:
            if self.correlation == "on_demand":  # the level rules alone: no volume is sized, none will exist
                N.corr_ondemand_layout(2 * B if stacked else B, enc.out_channels, h, w, self.correlation_pyramid_levels)
            else:
                N.corr_pyramid_layout(2 * B if stacked else B, h, w, self.correlation_pyramid_levels)
        except N.FtkError as e:
            raise ValueError(f"images of {H} x {W} give {h} x {w} feature maps, too small for {self.correlation_pyramid_levels} correlation levels: "
                             f"{e}") from None
        return n, B, H, W, h, w

    def _track(self, flow, mask, points, size, B: int, forward_backward, return_error: bool, return_flow: bool):
        """The end of a tracking call: the points launch on the loop's last flow and mask ([2B, ...] with the check: forward, then backward),
        and the result tuple as ``track_points`` documents it."""
        check = forward_backward is not None
        if check:
            result = track_points_from_flow(flow[:B], mask[:B], points, size, backward=(flow[B:], mask[B:]), forward_backward=forward_backward)
        else:
            result = track_points_from_flow(flow, mask, points, size)
        result = result if return_error else result[:2]
        return result + (((flow[:B], flow[B:]) if check else flow),) if return_flow else result

    def track_points(self, ref_image, cur_image, points, iterations: int = None, forward_backward: float = None, return_error: bool = False,
                     flow_init=None, return_flow: bool = False):
        """RAFT as a feature tracker: ``points`` [B, N, 2] (float32 CUDA, ``(x, y)`` pixels of ``ref_image``) give
        ``(cur_points [B, N, 2], status [B, N] uint8)``, the points in ``cur_image`` and their TrackStatus, as ``track_points_from_flow``
        defines them on the last iteration's coarse flow and mask with the images' own ``(H, W)`` as ``image_size``: bit for bit what
        sampling ``self(ref_image, cur_image)[-1]`` bilinearly at the points gives.  The loop is ``__call__``'s without the mask head in all
        but the last iteration and without any ``upsample_flow``: 36 + 14 * iterations - 2 * (iterations - 1) + 1 launches (a lookup and
        UpdateBlock's 13 per iteration).
        ``forward_backward=t`` (pixels, finite, >= 0) adds the forward-backward check: the feature encoder still runs once, the loop runs
        at batch 2B on the pair and the swapped pair, and the two halves of the last iteration are the forward and the backward flow of one
        launch; a tracked point that does not come back within ``t`` pixels is ``LARGE_RESIDUAL``.  ``return_error=True`` appends
        ``fb_error2`` [B, N] (``None`` without the check).  ``flow_init`` [B, 2, h, w] starts the loop from ``ref + flow_init`` as in
        ``__call__``; with the check it is a ``(forward_init, backward_init)`` pair.  ``return_flow=True`` appends the last iteration's
        coarse ``cur - ref`` [B, 2, h, w], with the check the pair ``(forward, backward)``.  Every argument is checked before the first
        launch; on torch's current stream, capturable at fixed shapes."""
        import torch

        check = forward_backward is not None
        if check and (not float(forward_backward) >= 0 or not math.isfinite(float(forward_backward))):
            raise ValueError(f"forward_backward must be a finite number of pixels >= 0 (got {forward_backward})")
        n, B, H, W, h, w = self._check_pair(ref_image, cur_image, points, iterations, check, flow_init)
        if check and flow_init is not None:
            flow_init = torch.cat([flow_init[0], flow_init[1]], dim=0)
        both = torch.cat([ref_image, cur_image], dim=0)
        features = self.feature_encoder(both, normalise=True)
        if check:  # entries 0 .. B - 1: ref -> cur; B .. 2B - 1: cur -> ref
            fmap0, fmap1 = features, torch.cat([features[B:], features[:B]], dim=0)
            inp, net = self.context_encoder(both, normalise=True)
        else:
            fmap0, fmap1 = features[:B], features[B:]
            inp, net = self.context_encoder(ref_image, normalise=True)
        flow, mask, _ = self._refine(fmap0, fmap1, inp, net, n, flow_init, "last")
        return self._track(flow, mask, points, (H, W), B, forward_backward, return_error, return_flow)


class RaftVideoTracker:
    """``Raft.track_points`` over a frame sequence.  ``track(image, points)`` treats the frame of the previous call as
    ``ref_image`` and ``image`` as ``cur_image`` and returns what ``raft.track_points(previous, image, points, iterations,
    forward_backward, return_error)`` returns, ``points`` in the previous frame's pixels; then ``image`` becomes the stored frame.
    Two things carry over from pair to pair.  The feature map: the feature encoder runs once per frame, on the new image at batch B,
    and the previous frame's map is kept (an output element of ``conv2d_kernel`` is one k-ordered ``fmaf`` chain whatever the batch, so
    the kept map is bit for bit the half of the stacked call's).  The flow, with ``warm_start=True``: a pair's loop starts from
    ``warm_start_flow`` of the previous pair's coarse flow, as upstream RAFT's video mode does, with the check each direction from its own;
    the first pair after construction or ``reset()`` starts from zero.  With ``warm_start=False`` every pair starts from zero and the
    results are ``track_points``' bit for bit.
    Launches per frame, ``track_points``' count with the encoder's 17 at batch B instead of 2B: 36 + 14 * iterations - 2 * (iterations - 1)
    + 1, plus ``warm_start_flow``'s one or two (one call over both directions of the check) from the second pair on; ``points=None``
    saves the points launch and the mask head's two.  The context encoder is not cached: it runs on the previous image (on both with the
    check), which is kept as a copy.  Not capturable as a whole: a call changes the state of the object."""

    def __init__(self, raft: Raft, iterations: int = None, warm_start: bool = True, forward_backward: float = None):
        if not isinstance(raft, Raft):
            raise ValueError(f"raft must be a Raft (got {type(raft).__name__})")
        n = raft.max_iterations if iterations is None else int(iterations)
        if n < 1:
            raise ValueError(f"iterations {iterations} must be at least 1")
        if forward_backward is not None and (not float(forward_backward) >= 0 or not math.isfinite(float(forward_backward))):
            raise ValueError(f"forward_backward must be a finite number of pixels >= 0 (got {forward_backward})")
        self.raft, self.iterations, self.warm_start = raft, n, bool(warm_start)
        self.forward_backward = None if forward_backward is None else float(forward_backward)
        self.reset()

    def reset(self) -> None:
        """Drops the stored frame and flow: the next ``track`` is a first call."""
        self._image, self._features, self._flow = None, None, None

    @property
    def last_flow(self):
        """The last pair's coarse flow [B, 2, h, w], with the check the pair ``(forward, backward)``; None before the second frame."""
        if self._flow is None or self.forward_backward is None:
            return self._flow
        B = self._flow.size(0) // 2
        return self._flow[:B], self._flow[B:]

    def track(self, image, points=None, return_error: bool = False):
        """The first call after construction or ``reset()`` encodes and stores ``image`` [B, in_channels, H, W] (float32 CUDA, 0 .. 255)
        and returns None.  Every later call returns ``(cur_points, status)``, with ``return_error=True`` and ``fb_error2``, of ``points``
        [B, N, 2] (pixels of the previous frame) in ``image``, or None for ``points=None``, which only advances the state.  A frame whose
        shape, dtype or device differs from the stored one is a ValueError.  Every argument is checked before the first launch."""
        import torch

        raft, check = self.raft, self.forward_backward is not None
        first = self._image is None
        channels = raft.feature_encoder.in_channels
        if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or image.dim() != 4 or image.size(1) != channels:
            got = f"{image.dtype} {list(image.shape)}" if isinstance(image, torch.Tensor) else type(image).__name__
            raise ValueError(f"image must be a 4-D float32 CUDA tensor [B, {channels}, H, W] (no CPU fallback, no other dtype): got {got}")
        if not first and (image.shape, image.device) != (self._image.shape, self._image.device):
            raise ValueError(f"this frame is {image.dtype} {list(image.shape)} on {image.device}, the stored one {self._image.dtype} "
                             f"{list(self._image.shape)} on {self._image.device}: call reset() before a sequence of another shape")
        previous = image if first else self._image
        _, B, H, W, _, _ = raft._check_pair(previous, image, None if first else points, self.iterations, check)
        features = raft.feature_encoder(image, normalise=True)
        if first:
            self._image, self._features = image.clone(), features
            return None
        if check:  # entries 0 .. B - 1: previous -> image; B .. 2B - 1: image -> previous
            fmap0, fmap1 = torch.cat([self._features, features], dim=0), torch.cat([features, self._features], dim=0)
            inp, net = raft.context_encoder(torch.cat([previous, image], dim=0), normalise=True)
        else:
            fmap0, fmap1 = self._features, features
            inp, net = raft.context_encoder(previous, normalise=True)
        flow_init = warm_start_flow(self._flow) if self.warm_start and self._flow is not None else None
        flow, mask, _ = raft._refine(fmap0, fmap1, inp, net, self.iterations, flow_init, "never" if points is None else "last")
        self._image, self._features, self._flow = image.clone(), features, flow
        if points is None:
            return None
        return raft._track(flow, mask, points, (H, W), B, self.forward_backward, return_error, False)
