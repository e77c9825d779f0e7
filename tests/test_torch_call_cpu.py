"""feature_tracker_amd/_torch_call.py without a device: the stream scope over a fake ``torch`` whose streams record what
is asked of them, the two workspace policies, the refusal of a context without a stream, and that importing the package leaves torch out."""
import os
import subprocess
import sys
import types

import pytest

from feature_tracker_amd import _torch_call as T
from feature_tracker_amd import device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_stream(self, other):
        self.log.append(f"{self.name}.wait({other.name})")


class _Guard:
    def __init__(self, stream, log):
        self.stream, self.log = stream, log

    def __enter__(self):
        self.log.append(f"enter({self.stream.name})")

    def __exit__(self, *exc):
        self.log.append(f"exit({self.stream.name})")
        return False


class _Tensor:
    def __init__(self, words, dtype, device):
        self.words, self.dtype, self.device = words, dtype, device

    def numel(self):
        return self.words


def _fake_torch(monkeypatch):
    """A ``torch`` that knows streams, guards and ``empty``; (the namespace, the log, the caller's stream)."""
    log = []
    caller = _Stream("caller", log)
    torch = types.SimpleNamespace(int64="int64", empty=lambda words, dtype, device: _Tensor(words, dtype, device),
                                  cuda=types.SimpleNamespace(current_stream=lambda device=None: caller, stream=lambda s: _Guard(s, log)))
    monkeypatch.setattr(D, "_torch", lambda: torch)
    return torch, log, caller


def test_one_stream_for_caller_and_context_waits_for_nothing(monkeypatch):
    torch, log, caller = _fake_torch(monkeypatch)
    tensor = types.SimpleNamespace(device="cuda:0")
    for ctx in (types.SimpleNamespace(handle=None, stream=caller), types.SimpleNamespace(handle=None)):  # its stream is the caller's; it has none
        del log[:]
        with T.OnStream(ctx, tensor) as on:
            log.append("body")
            assert on.ctx is ctx and on.stream is caller and on.torch is torch
        assert log == ["enter(caller)", "body", "exit(caller)"]


def test_two_streams_wait_for_each_other_around_the_guard(monkeypatch):
    _, log, caller = _fake_torch(monkeypatch)
    ctx = types.SimpleNamespace(handle=None, stream=_Stream("ctx", log))
    for where in (types.SimpleNamespace(device="cuda:0"), "cuda:0"):  # a tensor, or the device itself
        del log[:]
        with T.OnStream(ctx, where) as on:
            log.append("body")
            assert on.stream is ctx.stream and on.caller is caller
        assert log == ["ctx.wait(caller)", "enter(ctx)", "body", "exit(ctx)", "caller.wait(ctx)"]


def test_a_body_that_raises_leaves_the_guard_and_nobody_waits(monkeypatch):
    _, log, _ = _fake_torch(monkeypatch)
    ctx = types.SimpleNamespace(handle=None, stream=_Stream("ctx", log))
    error = KeyError("the body's own")
    with pytest.raises(KeyError) as caught:
        with T.OnStream(ctx, types.SimpleNamespace(device="cuda:0")):
            raise error
    assert caught.value is error
    assert log == ["ctx.wait(caller)", "enter(ctx)", "exit(ctx)"]


def test_no_context_means_the_default_context_of_the_tensors_device(monkeypatch):
    _fake_torch(monkeypatch)
    made = []
    monkeypatch.setattr(T, "Context", lambda index: made.append(index) or types.SimpleNamespace(handle=None, index=index))
    monkeypatch.setattr(T, "_contexts", {})
    tensor = types.SimpleNamespace(device=types.SimpleNamespace(index=3))
    first = T.OnStream(None, tensor).ctx
    assert first.index == 3 and T.OnStream(None, tensor).ctx is first and T.context_of(tensor) is first and T.context_of_index(3) is first
    assert made == [3]
    from feature_tracker_amd import raft
    assert raft._context is T.context_of_index and raft._device_context is T.context_of


def test_the_exact_holder_keeps_one_value_per_key(monkeypatch):
    torch, _, _ = _fake_torch(monkeypatch)
    holder, made = T.PerKey(), []

    def make(nbytes):
        made.append(nbytes)
        return T.words(torch, nbytes, "cuda:0")

    a = holder.of(("cuda:0", 6, 7), lambda: make(808))
    assert (a.words, a.dtype, a.device) == (101, "int64", "cuda:0")
    assert holder.of(("cuda:0", 6, 7), lambda: make(808)) is a and made == [808]
    b = holder.of(("cuda:0", 6, 8), lambda: make(801))
    assert b is not a and b.words == 101 and made == [808, 801]  # (bytes round up to words)
    assert holder.of(("cuda:0", 6, 7), lambda: make(808)) is a and set(holder) == {("cuda:0", 6, 7), ("cuda:0", 6, 8)}


def test_the_grown_holder_keeps_one_block_per_device(monkeypatch):
    torch, _, _ = _fake_torch(monkeypatch)
    holder = T.PerDevice()
    first = holder.of(torch, "cuda:0", 800)
    assert (first.words, first.dtype, first.device) == (125, "int64", "cuda:0")  # 100 words and a quarter
    assert holder.of(torch, "cuda:0", 1000) is first  # 125 words fit
    assert holder.of(torch, "cuda:0", 8) is first
    grown = holder.of(torch, "cuda:0", 1001)  # 126 words do not
    assert grown is not first and grown.words == 126 + 126 // 4 and holder["cuda:0"] is grown and len(holder) == 1
    assert holder.of(torch, "cuda:0", 800) is grown  # a smaller later request keeps the large block
    assert holder.of(torch, "cuda:1", 80).words == 12 and len(holder) == 2


def test_check_ctx_words_the_refusal_as_the_modules_did():
    T.check_ctx(None)
    T.check_ctx(types.SimpleNamespace(stream=object()))
    bare = types.SimpleNamespace(handle=None)
    with pytest.raises(ValueError) as refusal:
        T.check_ctx(bare)
    assert str(refusal.value) == ("ctx must come from device.context_on_stream(stream): torch must know the stream the kernels run on (None: torch's "
                                  "current stream)")
    with pytest.raises(ValueError) as refusal:
        T.check_ctx(bare, none_means="the tracker makes its own", because="the table's tensors are torch's, and ")
    assert str(refusal.value) == ("ctx must come from device.context_on_stream(stream): the table's tensors are torch's, and torch must know the stream "
                                  "the kernels run on (None: the tracker makes its own)")


def test_the_modules_refuse_with_those_words():
    import feature_tracker_amd as F
    bare = types.SimpleNamespace(handle=None)
    usual = "ctx must come from device.context_on_stream(stream): torch must know the stream the kernels run on (None: torch's current stream)"
    for make in (lambda: F.EpipolarRansac(ctx=bare), lambda: F.TwoViewRansac(ctx=bare), lambda: F.KeypointDecoder(ctx=bare),
                 lambda: F.MatchAssignment.without_weights(8, ctx=bare), lambda: F.SuperPoint({}, ctx=bare), lambda: F.attention(None, None, None, ctx=bare)):
        with pytest.raises(ValueError) as refusal:
            make()
        assert str(refusal.value) == usual
    with pytest.raises(ValueError) as refusal:
        F.KltVideoTracker(F.OpticalFlowBasicKlt(), 8, ctx=bare)
    assert str(refusal.value) == ("ctx must come from device.context_on_stream(stream): the table's tensors are torch's, and torch must know the stream "
                                  "the kernels run on (None: the tracker makes its own)")


def test_call_raises_the_contexts_error_only_for_a_nonzero_return(monkeypatch):
    from feature_tracker_amd import _native as N
    seen = []
    lib = types.SimpleNamespace(ftk_fine=lambda *args: seen.append(args) or 0, ftk_refused=lambda *args: -1, ftk_last_error=lambda handle: b"what went wrong")
    monkeypatch.setattr(N, "lib", lambda: lib)
    T.call("ftk_fine", (1, 2), types.SimpleNamespace(handle=None))
    assert seen == [(1, 2)]
    with pytest.raises(N.FtkError, match="what went wrong"):
        T.call("ftk_refused", (), types.SimpleNamespace(handle=None))


def test_pointer_and_stream_or_current(monkeypatch):
    _, _, caller = _fake_torch(monkeypatch)
    tensor = types.SimpleNamespace(device="cuda:0", data_ptr=lambda: 0x4000)
    assert T.pointer(None) is None and T.pointer(tensor).value == 0x4000
    given = object()
    assert T.stream_or_current(tensor, given) is given and T.stream_or_current(tensor, None) is caller


def test_importing_the_package_leaves_torch_out():
    code = "import sys, feature_tracker_amd, feature_tracker_amd._torch_call; sys.exit(1 if 'torch' in sys.modules else 0)"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
