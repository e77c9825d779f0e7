"""What the argument tests of the torch device entries share (tests/test_device_args_cpu.py and the tests/test_*_args_cpu.py files).

TEST INFRASTRUCTURE ONLY.  The walk: duck-typed tensors whose ``data_ptr()`` tells on a caller that did not have them checked first, and a
recording stand-in for the native library, so an entry runs to its native call without a device.  The helpers below are the assertions
every file made in its own copy; a file states what is its own: the call, the expected native entries, the kinds it walks, the names
that get the loose match, its constants and symbols, and its plan restatement.
"""
import os
import re
import subprocess
import types

import pytest

import feature_tracker_amd as F
from feature_tracker_amd import _native as N
from feature_tracker_amd import device as D
from feature_tracker_amd import dist as FD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeDtype:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "torch." + self.name


_DTYPES = {n: FakeDtype(n) for n in ("float32", "uint8", "int32", "uint32", "int64")}


class FakeDevice:
    type = "cuda"

    def __init__(self, index=0):
        self.index = index

    def __eq__(self, other):
        return isinstance(other, FakeDevice) and other.index == self.index

    def __repr__(self):
        return f"cuda:{self.index}"


class Fake:
    """What device.py may ask of a tensor, and a ``data_ptr()`` that tells on a caller who did not have the tensor checked first."""
    is_cuda = True

    def __init__(self, name, dtype, shape, checked, unchecked_reads, device=None):
        self.name, self.dtype, self.shape, self.device = name, _DTYPES[dtype], tuple(shape), device or FakeDevice(0)
        self._checked, self._unchecked_reads, self.reads = checked, unchecked_reads, 0

    def stride(self, k=None):
        s, run = [], 1
        for e in reversed(self.shape):
            s.append(run)
            run *= e
        s = tuple(reversed(s))
        return s if k is None else s[k]

    def size(self, k=None):
        return self.shape if k is None else self.shape[k]

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for e in self.shape:
            n *= e
        return n

    def is_contiguous(self):
        return True

    def data_ptr(self):
        self.reads += 1
        if id(self) not in self._checked:
            self._unchecked_reads.append(self.name)
        return 0x10000


class RecorderLib:
    """Stands where the loaded library stands: every entry point is recorded and answers FTK_OK; nothing is launched."""

    def __init__(self):
        self.calls = []

    def ftk_klt_shard_bytes(self, n, world):
        return FD.packed_bytes(FD.shard_capacity(n, world)) if n > 0 and world > 0 else 0

    def __getattr__(self, name):
        if not name.startswith("ftk_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            return 0

        return entry


class FakePyramid:
    handle = None

    def level_desc(self, i):
        return 0, 12, 16

    @classmethod
    def from_device_levels(cls, desc, ctx, keepalive=None):
        N.lib().ftk_pyramid_wrap_device(desc)
        return cls()


def one_row_fewer(fake):
    return (fake.shape[0] - 1,) + fake.shape[1:]


def one_row_more(fake):
    return (fake.shape[0] + 1,) + fake.shape[1:]


def one_column_more(fake):
    return fake.shape[:-1] + (fake.shape[-1] + 1,)


class Walk:
    """``spoil=(k, kind, value)`` makes the k-th tensor of the walk wrong: ``kind`` "dtype" gives it the dtype named ``value`` (float64
    for None), "shape" the shape ``value`` or ``value(fake)``, "device" the device index ``value`` (1 for None).  ``spoiled`` is then
    that tensor."""

    def __init__(self, monkeypatch, spoil=None):
        self.checked, self.unchecked_reads, self.made = set(), [], []
        self.spoil, self.spoiled = spoil, None
        self.lib = RecorderLib()
        real_check = D._check

        def recording_check(name, t, *args, **kwargs):
            real_check(name, t, *args, **kwargs)
            self.checked.add(id(t))

        stream = types.SimpleNamespace(cuda_stream=0)
        fake_torch = types.SimpleNamespace(cuda=types.SimpleNamespace(current_stream=lambda device=None: stream))
        monkeypatch.setattr(D, "_check", recording_check)
        monkeypatch.setattr(D, "_torch", lambda: fake_torch)
        monkeypatch.setattr(D, "ImagePyramid", FakePyramid)
        monkeypatch.setattr(N, "lib", lambda: self.lib)
        monkeypatch.setattr(N, "corr_pyramid_layout", lambda B, H, W, levels: (B * H * W * H * W * levels, [], []))
        self.ctx = types.SimpleNamespace(handle=None, device_index=0)
        self.comm = types.SimpleNamespace(handle=None)
        self.pyr = FakePyramid()

    def t(self, name, dtype, *shape):
        fake = Fake(name, dtype, shape, self.checked, self.unchecked_reads)
        if self.spoil is not None and len(self.made) == self.spoil[0]:
            _, kind, value = self.spoil
            if kind == "dtype":
                fake.dtype = FakeDtype(value or "float64")
            elif kind == "shape":
                fake.shape = tuple(value(fake) if callable(value) else value)
            else:
                assert kind == "device", kind
                fake.device = FakeDevice(1 if value is None else value)
            self.spoiled = fake
        self.made.append(fake)
        return fake

    def klt(self):
        return D.DeviceKlt("basic", F.OpticalFlowOptions(), self.pyr, self.pyr, self.ctx)

    def klt_in(self, n=8):
        return self.t("ref_uv", "float32", n, 2), self.t("cur_uv_in", "float32", n, 2), self.t("status_in", "uint8", n)

    def klt_out(self, n=8):
        return self.t("cur_uv_out", "float32", n, 2), self.t("status_out", "uint8", n)

    def nearby(self, n_ref=8, n_cur=9):
        return dict(pred_uv=self.t("pred_uv", "float32", n_ref, 2), cur_uv=self.t("cur_uv", "float32", n_cur, 2))


def walk_call(monkeypatch, call, calls):
    """``call(w)`` with every argument right: no ``data_ptr()`` of an unchecked tensor, exactly the native entries ``calls``, and every
    tensor the call made read exactly once.  Returns the walk."""
    w = Walk(monkeypatch)
    call(w)
    assert w.unchecked_reads == [], f"data_ptr() of {w.unchecked_reads} taken without a check"
    assert w.lib.calls == calls
    assert [f.name for f in w.made if f.reads != 1] == []
    return w


def refused_call(monkeypatch, call, spoil, match):
    """``call(w)`` with one tensor spoiled (see Walk): ValueError matching ``match``, no library call and no unchecked read."""
    w = Walk(monkeypatch, spoil=spoil)
    with pytest.raises(ValueError, match=match):
        call(w)
    assert w.lib.calls == [] and w.unchecked_reads == []
    return w


def refusal_sweep(monkeypatch, call, kind, loose=(), reshape=one_row_fewer, skip=()):
    """Each tensor ``call(w)`` makes, in order, spoiled in ``kind`` ("shape" through ``reshape``): refused as ``^{name} must be``, or as
    plain ``must be`` for a "shape" of a name in ``loose``; a "shape" of a name in ``skip`` is not tried.  Returns the tensors' names."""
    probe = Walk(monkeypatch)
    call(probe)
    for k, made in enumerate(probe.made):
        if kind == "shape" and made.name in skip:
            continue
        match = "must be" if kind == "shape" and made.name in loose else f"^{made.name} must be"
        refused_call(monkeypatch, call, (k, kind, reshape if kind == "shape" else None), match)
    return [made.name for made in probe.made]


def header_library_and_binding_agree(constants, symbols):
    """include/ftk.h, the binding's constants and the export list say the same.  Returns the header's text."""
    header = open(os.path.join(ROOT, "include", "ftk.h")).read()
    for name in constants:
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == getattr(N, name), name
    assert int(re.search(r"#define FTK_ABI_VERSION (\d+)", header).group(1)) == 1
    assert set(symbols) <= set(N.EXPORTS), set(symbols) - set(N.EXPORTS)
    for s in symbols:
        assert re.search(rf"\bint {s}\(", header), s
    return header


def nothing_in_the_package_imports(word):
    for folder, _, files in os.walk(os.path.join(ROOT, "feature_tracker_amd")):
        for f in files:
            if f.endswith(".py"):
                assert word not in open(os.path.join(folder, f)).read(), f


def plan_cli(name):
    return os.path.join(ROOT, "feature_tracker_amd", "host", "build", name)


def run_plan_tool(exe, cases, timeout=None):
    """One line of space-separated values per case into the plan tool; one ``{key: str}`` dict per case back."""
    assert os.path.exists(exe), f"host/build/{os.path.basename(exe)} is missing: build() makes it"
    text = "".join(" ".join(str(v) for v in c) + "\n" for c in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=timeout).stdout.strip().split("\n")
    assert len(out) == len(cases)
    return [dict(kv.split("=") for kv in line.split()) for line in out]
