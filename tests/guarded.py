"""Guarded memory for the tests that hold a device entry to the sizes it declares: every tensor a call may write (and every tensor it
only reads) is a payload of exactly its documented size inside ONE flat uint8 arena, ``[guard | payload | guard | payload | ... | guard]``.
A write past a payload lands in a guard band of the same allocation and ``check()`` names it; a result that depends on what a payload
held before the call shows when the same arena is built twice, from an all-zeros and from an all-ones fill.

The bands are at least as large as the payload next to them (up to 1 MiB), so that an overrun by a whole row or plane still ends in a
band.  Every payload starts on a 256-byte boundary of the address space, as a block of torch's caching allocator does: an entry sees
the alignment it sees from its usual callers.

TEST INFRASTRUCTURE ONLY: torch and numpy; works on CPU tensors (tests/test_guarded_cpu.py) as on CUDA ones.
"""
from __future__ import annotations

import numpy as np

GUARD_BYTE = 0xA5
MIN_GUARD = 4096          # bytes of every band at least
MAX_GUARD = 1 << 20       # a band follows its neighbours' size up to here
ALIGN = 256               # of every payload's address
ZEROS, ONES = 0x00, 0xFF  # the two payload fills of a poison pair: +0.0 / 0 / false, and NaN / -1 / an all-ones key


class GuardDamaged(AssertionError):
    """A guard band does not hold its pattern.  ``before`` / ``after``: the names of the payloads on either side of the band (None at an
    end of the arena); ``first`` / ``last``: the arena offsets of the first and the last damaged byte; ``past_before``: bytes from the end
    of ``before`` to ``first`` (0: the byte right behind it); ``ahead_of_after``: bytes from ``last`` to the start of ``after`` (1: the
    byte right in front of it)."""

    def __init__(self, before, after, first, last, past_before, ahead_of_after, damaged):
        self.before, self.after, self.first, self.last = before, after, first, last
        self.past_before, self.ahead_of_after, self.damaged = past_before, ahead_of_after, damaged
        where = []
        if before is not None:
            where.append(f"starts {past_before} bytes past the end of '{before}'")
        if after is not None:
            where.append(f"ends {ahead_of_after} bytes ahead of the start of '{after}'")
        super().__init__(f"the guard between {before!r} and {after!r} was written: {damaged} bytes changed, arena offsets {first} .. {last}; the damage "
                         + " and ".join(where))


def _up(v, to):
    return -(-int(v) // to) * to


def _torch_dtype(torch, dtype):
    return getattr(torch, dtype) if isinstance(dtype, str) else dtype


class Arena:
    """``Arena([(name, dtype, shape, fill_byte), ...], device)``: the payloads back to back in the order given, each between two guard bands.
    ``dtype``: a torch dtype or its name.  ``fill``: one byte for every payload instead of its own ``fill_byte``.  ``arena[name]`` is the
    typed, contiguous view of a payload (``.view(dtype)`` of a slice of the arena: its ``data_ptr()`` is the payload's first byte, its
    ``numel`` exactly the shape's)."""

    def __init__(self, specs, device="cpu", fill=None):
        import torch

        self.names, self.spans, self.fills, self.views = [], {}, {}, {}
        sized = []
        for name, dtype, shape, fill_byte in specs:
            dtype = _torch_dtype(torch, dtype)
            shape = tuple(int(e) for e in shape)
            nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
            assert nbytes > 0 and name not in self.spans and all(e > 0 for e in shape), (name, shape)
            sized.append((name, dtype, shape, nbytes, int(fill_byte if fill is None else fill) & 0xFF))
            self.spans[name] = None
        band = lambda nbytes: max(MIN_GUARD, min(nbytes, MAX_GUARD))  # noqa: E731
        at = 0
        for k, (name, dtype, shape, nbytes, _) in enumerate(sized):
            least = band(nbytes) if k == 0 else max(band(nbytes), band(sized[k - 1][3]))
            at = _up(at + least, ALIGN)
            self.spans[name] = (at, at + nbytes)
            at += nbytes
        total = at + band(sized[-1][3])
        # the base on a 256-byte boundary whatever the allocator gives (torch's CPU allocator aligns to 64 bytes)
        raw = torch.empty(total + ALIGN, dtype=torch.uint8, device=device)
        shift = -raw.data_ptr() % ALIGN
        self.raw = raw
        self.buf = raw[shift:shift + total]
        assert self.buf.data_ptr() % ALIGN == 0 and self.buf.numel() == total and self.buf.is_contiguous()
        self.total = total
        self.buf.fill_(GUARD_BYTE)
        for name, dtype, shape, nbytes, fill_byte in sized:
            a, b = self.spans[name]
            self.buf[a:b].fill_(fill_byte)
            view = self.buf[a:b].view(dtype).view(shape)
            assert view.is_contiguous() and view.data_ptr() == self.buf.data_ptr() + a and view.data_ptr() % ALIGN == 0
            assert view.numel() * view.element_size() == nbytes and tuple(view.shape) == shape
            self.names.append(name)
            self.fills[name] = fill_byte
            self.views[name] = view

    def __getitem__(self, name):
        return self.views[name]

    def span(self, name):
        """(first byte, one past the last byte) of a payload, as arena offsets."""
        return self.spans[name]

    def put(self, name, array):
        """Copies a numpy array of the payload's shape and element size into it (an input of the call under test); returns the view."""
        import torch

        view = self.views[name]
        array = np.ascontiguousarray(array)
        assert tuple(array.shape) == tuple(view.shape) and array.dtype.itemsize == view.element_size(), (name, array.shape, array.dtype)
        view.copy_(torch.from_numpy(array.copy()).view(view.dtype))
        return view

    def payload_mask(self) -> np.ndarray:
        """bool [total]: True on payload bytes, False on guard bytes."""
        mask = np.zeros(self.total, bool)
        for a, b in self.spans.values():
            mask[a:b] = True
        return mask

    def host(self) -> np.ndarray:
        """The whole arena on the host, one copy."""
        return self.buf.cpu().numpy().copy()

    def payload_bytes(self, name, host=None) -> np.ndarray:
        a, b = self.spans[name]
        return (self.host() if host is None else host)[a:b]

    def check(self, host=None):
        """One copy of the arena to the host; GuardDamaged for the first band (in address order) that does not hold its pattern."""
        host = self.host() if host is None else host
        for k in range(len(self.names) + 1):
            before = self.names[k - 1] if k > 0 else None
            after = self.names[k] if k < len(self.names) else None
            a = self.spans[before][1] if before is not None else 0
            b = self.spans[after][0] if after is not None else self.total
            bad = np.flatnonzero(host[a:b] != GUARD_BYTE)
            if bad.size:
                first, last = a + int(bad[0]), a + int(bad[-1])
                raise GuardDamaged(before, after, first, last, first - a, b - last, int(bad.size))
        return host


def poison_pair(specs, device="cpu"):
    """The same arena twice: every payload all 0x00, and every payload all 0xFF (NaN as float32, -1 as int32, an all-ones key)."""
    return Arena(specs, device, fill=ZEROS), Arena(specs, device, fill=ONES)


def same_bytes(tensor, array) -> bool:
    """A tensor holds exactly the bytes of a numpy array of its shape (an input that the call must leave as it was)."""
    got = tensor.detach().cpu().contiguous().numpy()
    array = np.ascontiguousarray(array)
    return got.shape == array.shape and got.dtype.itemsize == array.dtype.itemsize and got.tobytes() == array.tobytes()
