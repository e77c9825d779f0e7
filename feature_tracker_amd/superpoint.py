"""``SuperPoint``: the network in front of ``KeypointDecoder`` on the device.

SuperPoint (DeTone, Malisiewicz, Rabinovich 2018) is a small VGG: eight 3 x 3 convolutions with ReLU, three 2 x 2 max-pools and two heads of
one 3 x 3 and one 1 x 1 layer each.  Every convolution is ``conv2d_kernel``; the three pools run in the epilogue of the
layer before them (``device.conv2d_pool_device``), and the L2 normalisation of the dense descriptor map writes the channel-last layout
``KeypointDecoder.decode`` reads fastest (``device.channel_normalise_device``).  One image is twelve launches on one stream, no host read.

Inference only, float32 only, one image per call, no CPU fallback.  No trained weights come with this package.
"""
from __future__ import annotations

from typing import Dict, Mapping

from . import _native as N
from . import device as D
from ._torch_call import OnStream, PerKey, check_ctx
from .raft import _check_no_grad, _pack_conv, _state_tensor

# upstream's layer names in forward order: (name, kernel size)
TRUNK = (("conv1a", 3), ("conv1b", 3), ("conv2a", 3), ("conv2b", 3), ("conv3a", 3), ("conv3b", 3), ("conv4a", 3), ("conv4b", 3))
HEADS = (("convPa", 3), ("convPb", 1), ("convDa", 3), ("convDb", 1))
POOLED = ("conv1b", "conv2b", "conv3b")  # the layers with a max-pool after their ReLU
SEMI_CHANNELS = 65                       # 64 pixels of a cell and the dustbin
CELL = N.FTK_KEYPOINT_DECODE_CELL
LAUNCHES = 12


class SuperPoint:
    """``SuperPoint.from_state_dict(sd, prefix="")`` reads upstream's names (``conv1a`` ... ``conv4b``, ``convPa``, ``convPb``, ``convDa``,
    ``convDb``, each with ``.weight`` / ``.bias``); all widths are read off the weights.

    ``heads(image)`` -> ``(semi [65, Hc, Wc], desc [D, Hc, Wc])`` for a float32 CUDA ``image`` [H, W] or [1, 1, H, W] in 0 .. 1 with H, W
    multiples of 8: the detector head's logits and the L2-normalised dense descriptors, ``desc`` as the ``permute(2, 0, 1)`` view of a
    contiguous [Hc, Wc, D] tensor.  Both are this object's buffers of that image size: they are valid, in stream order, until the next call
    of the size.  ``detect(image, decoder)`` is ``decoder.decode(*heads(image))``.

    ``convPa`` and ``convDa`` read the same tensor and run as one layer of their stacked output channels; ``convPb`` and ``convDb`` read
    its two channel halves in place.  The kernels run on torch's current stream (or on ``ctx``'s, from ``device.context_on_stream``).  The
    intermediates are allocated once per image size and kept, so a pass is capturable in ``torch.cuda.graph`` after one call of the size."""

    def __init__(self, state: Mapping, prefix: str = "", ctx=None):
        import torch

        check_ctx(ctx)
        self._ctx = ctx
        taken, device, previous = {}, None, 1  # the image is one channel
        trunk_out = None
        for name, ks in TRUNK + HEADS:
            key = f"{prefix}{name}.weight"
            w = _state_tensor(state, key, 4)
            if name in ("convPa", "convDa"):
                previous = trunk_out
            M = int(w.shape[0])
            if tuple(w.shape) != (M, previous, ks, ks) or M < 1:
                raise ValueError(f"{key} must be a float32 tensor of shape [out_channels, {previous}, {ks}, {ks}] (got {w.dtype} {list(w.shape)})")
            if name == "convPb" and M != SEMI_CHANNELS:
                raise ValueError(f"{key} must have {SEMI_CHANNELS} output channels, the 64 pixels of a cell and the dustbin (got {M})")
            limit = N.FTK_KEYPOINT_DECODE_MAX_CHANNELS if name == "convDb" else N.FTK_CONV2D_MAX_OUT_CHANNELS
            if M > limit or previous > N.FTK_CONV2D_MAX_IN_CHANNELS:
                raise ValueError(f"{key}: a {ks} x {ks} convolution of {previous} -> {M} channels is outside the supported sizes (up to "
                                 f"{N.FTK_CONV2D_MAX_IN_CHANNELS} -> {limit} channels)")
            for kind, shape in (("weight", (M, previous, ks, ks)), ("bias", (M,))):
                key = f"{prefix}{name}.{kind}"
                t = _state_tensor(state, key)
                if t.dtype != torch.float32 or tuple(t.shape) != shape:
                    raise ValueError(f"{key} must be a float32 tensor of shape {list(shape)} (got {t.dtype} {list(t.shape)})")
                device = t.device if device is None else device
                if t.device != device:
                    raise ValueError(f"{key} is on {t.device}, the other weights on {device}")
                taken[f"{name}.{kind}"] = t.detach()
            previous = M
            if name == "conv4b":
                trunk_out = M
        self.weights: Dict[str, object] = taken
        self.widths = {name: int(taken[f"{name}.weight"].shape[0]) for name, _ in TRUNK + HEADS}
        self.detector_hidden, self.descriptor_hidden = self.widths["convPa"], self.widths["convDa"]
        self.descriptor_channels = self.widths["convDb"]
        if self.detector_hidden + self.descriptor_hidden > N.FTK_CONV2D_MAX_OUT_CHANNELS:
            raise ValueError(f"{prefix}convDa.weight: convPa and convDa run as one layer of {self.detector_hidden} + {self.descriptor_hidden} output channels, "
                             f"above FTK_CONV2D_MAX_OUT_CHANNELS = {N.FTK_CONV2D_MAX_OUT_CHANNELS}")
        # per launch: (packed weights, bias, kernel size, out_channels); each layer is packed once, convPa and convDa as one
        self._layers = {}
        for name, ks in TRUNK + (("convPb", 1), ("convDb", 1)):
            self._layers[name] = (_pack_conv(taken[f"{name}.weight"]), taken[f"{name}.bias"].contiguous(), ks, self.widths[name])
        stacked = torch.cat([taken["convPa.weight"], taken["convDa.weight"]], 0)
        self._layers["convPa+convDa"] = (_pack_conv(stacked), torch.cat([taken["convPa.bias"], taken["convDa.bias"]], 0).contiguous(), 3,
                                         self.detector_hidden + self.descriptor_hidden)
        self._device = device
        self._buffers = PerKey()  # (device, H, W) -> the tensors of a pass at that size

    @classmethod
    def from_state_dict(cls, state: Mapping, prefix: str = "", ctx=None):
        return cls(state, prefix, ctx)

    def buffer_shapes(self, H: int, W: int) -> Dict[str, tuple]:
        """The tensors one pass over an H x W image writes, in launch order: name -> shape."""
        w = self.widths
        shapes, h, ww = {}, H, W
        for k in (1, 2, 3):
            shapes[f"conv{k}a"] = (1, w[f"conv{k}a"], h, ww)
            h, ww = h // 2, ww // 2
            shapes[f"conv{k}b"] = (1, w[f"conv{k}b"], h, ww)
        shapes["conv4a"], shapes["conv4b"] = (1, w["conv4a"], h, ww), (1, w["conv4b"], h, ww)
        shapes["convPa+convDa"] = (1, self.detector_hidden + self.descriptor_hidden, h, ww)
        shapes["convPb"], shapes["convDb"] = (1, SEMI_CHANNELS, h, ww), (1, self.descriptor_channels, h, ww)
        shapes["desc"] = (h, ww, self.descriptor_channels)
        return shapes

    def _allocate(self, H: int, W: int, device):
        torch = D._torch()
        bufs = {name: torch.empty(shape, dtype=torch.float32, device=device) for name, shape in self.buffer_shapes(H, W).items()}
        # the two heads' inputs: channel halves of one image's tensor, which are dense
        bufs["convPa"], bufs["convDa"] = bufs["convPa+convDa"][:, :self.detector_hidden], bufs["convPa+convDa"][:, self.detector_hidden:]
        bufs["convDb[0]"] = bufs["convDb"][0]
        return bufs

    def _forward(self, ctx, image, bufs, stream=None) -> None:
        """The twelve launches over checked arguments: ``image`` [1, 1, H, W], ``bufs`` as ``_allocate`` makes them."""
        x = image
        for name, _ in TRUNK:
            weights, bias, ks, _ = self._layers[name]
            if name in POOLED:
                D.conv2d_pool_device(ctx, [x], weights, bias, ks, True, bufs[name], stream)
            else:
                D.conv2d_device(ctx, [x], weights, bias, ks, True, 1.0, bufs[name], stream)
            x = bufs[name]
        weights, bias, ks, _ = self._layers["convPa+convDa"]
        D.conv2d_device(ctx, [x], weights, bias, ks, True, 1.0, bufs["convPa+convDa"], stream)
        for name, source in (("convPb", "convPa"), ("convDb", "convDa")):
            weights, bias, ks, _ = self._layers[name]
            D.conv2d_device(ctx, [bufs[source]], weights, bias, ks, False, 1.0, bufs[name], stream)
        D.channel_normalise_device(ctx, bufs["convDb[0]"], bufs["desc"], stream)

    def _check_image(self, image):
        import torch

        if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or image.dim() not in (2, 4) or (image.dim() == 4 and tuple(image.shape[:2]) != (1, 1)):
            got = f"{image.dtype} {list(image.shape)}" if isinstance(image, torch.Tensor) else type(image).__name__
            raise ValueError(f"image must be a float32 CUDA tensor [H, W] or [1, 1, H, W] (one image, no CPU fallback, no other dtype): got {got}")
        H, W = int(image.shape[-2]), int(image.shape[-1])
        if H < CELL or W < CELL or H % CELL or W % CELL:
            raise ValueError(f"image must be a multiple of {CELL} and at least {CELL} along both axes (got {H} x {W}): a cell of the heads is {CELL} x {CELL} pixels")
        if not image.is_contiguous():
            raise ValueError(f"image must be contiguous (got strides {list(image.stride())}); nothing is copied here")
        _check_no_grad(torch, image, what="SuperPoint")
        if not image.is_cuda:
            raise ValueError(f"image must be a CUDA tensor (got one on {image.device}): there is no CPU fallback")
        if self._device != image.device:
            raise ValueError(f"the weights are on {self._device}, the image on {image.device}")
        return H, W

    def heads(self, image):
        """One image to the two head tensors ``KeypointDecoder.decode`` takes.  Everything is enqueued; nothing is read on the host."""
        H, W = self._check_image(image)
        device = image.device
        with OnStream(self._ctx, image) as on:
            bufs = self._buffers.of((device, H, W), lambda: self._allocate(H, W, device))
            self._forward(on.ctx, image.view(1, 1, H, W), bufs, on.stream)
        return bufs["convPb"][0], bufs["desc"].permute(2, 0, 1)

    def detect(self, image, decoder, occupied=None, occupied_mask=None, return_heatmap: bool = False):
        """``decoder.decode(*self.heads(image), ...)``: a ``KeypointResult`` on the device."""
        semi, desc = self.heads(image)
        return decoder.decode(semi, desc, occupied=occupied, occupied_mask=occupied_mask, return_heatmap=return_heatmap)
