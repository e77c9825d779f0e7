"""What every torch-facing call of this package does around its launches, stated once: the default context of a tensor's
device, the refusal of a context torch does not know the stream of, the stream scope, the complaints about tensors, the two workspace
policies, the checked native call, and the pointer and stream arguments of the ``_device_*.py`` entries.

Plain functions and three small classes; the modules keep their shapes, limits, result objects and docstrings.  Nothing here imports
torch: it is ``device._torch()``'s, asked for at each call.
"""
from __future__ import annotations

import ctypes as C

from . import _native as N
from .tracker import Context

_contexts = {}  # device index -> the one library context of that device
_device = None  # feature_tracker_amd.device, once asked for


def _D():
    """``feature_tracker_amd.device``.  It imports this module, so it is not imported here at import time; it is looked up at each call
    because its ``_torch`` is what says whether there is a HIP device."""
    global _device
    if _device is None:
        from . import device

        _device = device
    return _device


def context_of_index(index: int) -> Context:
    """One library context per device: it selects the device and records errors; the launches go to torch's current stream."""
    ctx = _contexts.get(index)
    if ctx is None:
        ctx = _contexts[index] = Context(index)
    return ctx


def context_of(tensor) -> Context:
    """``context_of_index`` of the device ``tensor`` is on."""
    index = tensor.device.index
    if index is None:
        index = _D()._torch().cuda.current_device()
    return context_of_index(index)


def check_ctx(ctx, none_means: str = "torch's current stream", because: str = "") -> None:
    """Refuses a context that ``device.context_on_stream`` did not make: only those say which torch stream their kernels run on."""
    if ctx is not None and getattr(ctx, "stream", None) is None:
        raise ValueError(f"ctx must come from device.context_on_stream(stream): {because}torch must know the stream the kernels run on (None: {none_means})")


class OnStream:
    """The context and stream of a call, and the scope its launches and allocations run in.  ``ctx`` None: the default context of
    ``where`` (a tensor, or its device when ``ctx`` is given).  The stream is ``ctx``'s where it has one, else the caller's, which is
    torch's current stream of the device.  Entering makes the stream wait for the caller's and enters ``torch.cuda.stream(stream)``;
    leaving leaves that guard and makes the caller's stream wait for the work, on the device.  Neither wait happens when the two are one
    stream, nor the second when the body raised."""

    __slots__ = ("torch", "ctx", "caller", "stream", "_apart", "_guard")

    def __init__(self, ctx, where):
        self.torch = _D()._torch()
        self.ctx = context_of(where) if ctx is None else ctx
        self.caller = self.torch.cuda.current_stream(getattr(where, "device", where))
        self.stream = getattr(self.ctx, "stream", None) or self.caller
        self._apart = self.stream != self.caller

    def __enter__(self):
        if self._apart:
            self.stream.wait_stream(self.caller)
        self._guard = self.torch.cuda.stream(self.stream)
        self._guard.__enter__()
        return self

    def __exit__(self, *exc):
        self._guard.__exit__(*exc)
        if self._apart and exc[0] is None:
            self.caller.wait_stream(self.stream)
        return False


def complain(tensors, cuda: bool = True) -> None:
    """``device._tensor_complaint`` of (name, tensor, dtypes, shape) in turn, then (``cuda``) that each is a CUDA tensor."""
    tensor_complaint = _D()._tensor_complaint
    for name, t, dtypes, shape in tensors:
        complaint = tensor_complaint(name, t, dtypes, shape)
        if complaint:
            raise ValueError(complaint)
    if cuda:
        complain_cuda((name, t) for name, t, _, _ in tensors)


def complain_cuda(named) -> None:
    for name, t in named:
        if not t.is_cuda:
            raise ValueError(f"{name} must be a CUDA tensor (got one on {t.device}): there is no CPU fallback")


def words(torch, nbytes: int, device):
    """A workspace of ``nbytes`` as the entries take it: int64 words."""
    return torch.empty(-(-nbytes // 8), dtype=torch.int64, device=device)


class PerKey(dict):
    """The exact policy: one value per key, say (device, M, N), made by the first call of that key and kept, so a call captured after one
    eager call of a size allocates nothing but its outputs.  Ask inside the stream scope."""

    def of(self, key, make):
        value = self.get(key)
        if value is None:
            value = self[key] = make()
        return value


class PerDevice(dict):
    """The grown policy: ONE workspace per device, replaced by one a quarter beyond the call's need when that call needs more, so a
    caller whose sizes change from call to call does not accumulate blocks.  Ask inside the stream scope: the block that is replaced
    goes back to torch's allocator in stream order."""

    def of(self, torch, device, nbytes: int):
        need = -(-nbytes // 8)
        block = self.get(device)
        if block is None or block.numel() < need:
            block = self[device] = torch.empty(need + need // 4, dtype=torch.int64, device=device)
        return block


def call(entry: str, args, ctx) -> None:
    """The native ``entry`` over marshalled ``args``; a nonzero return raises the context's last error."""
    rc = getattr(N.lib(), entry)(*args)
    if rc != 0:
        N.check(rc, ctx.handle)


def pointer(x):
    """A checked tensor as the C ABI takes it; None stays None."""
    return None if x is None else C.c_void_p(x.data_ptr())


def stream_or_current(tensor, stream):
    """The stream argument of an entry, or torch's current stream of ``tensor``'s device."""
    return stream if stream is not None else _D()._torch().cuda.current_stream(tensor.device)
