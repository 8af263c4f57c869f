"""Call trace of tripled_amd.ops on the CPU: every op is driven forward and backward against a stand-in library
(tests/ops_calls_util.py) and the C-ABI calls it makes -- names, order, argument counts, which tensor (dtype, shape, strides) sits
in which pointer slot, every scalar -- must equal tests/golden/ops_calls.json, recorded by tools/gen_golden_ops_calls.py.  A slip
in the marshalling of ops.py / native.py shows here in seconds; what the trace cannot see (two operands of identical dtype, shape
and strides swapped; the kernels themselves) is the GPU tests' business.  Also: native.call refuses bad arguments before the
library is touched."""
import json
import os

import pytest
import torch

from . import ops_calls_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ops_call_trace_equals_golden(monkeypatch):
    with open(U.golden_path(ROOT)) as f:
        golden = json.load(f)
    trace = json.loads(U.dumps(U.record(monkeypatch.setattr)))
    assert [c[0] for c in trace] == [c[0] for c in golden]
    for got, want in zip(trace, golden):
        assert got[1] == want[1], "calls of case %r" % got[0]
        assert got[2] == want[2], "dispatch counters of case %r" % got[0]
    assert sum(len(c[1]) for c in trace) > 500


@pytest.fixture
def stub(monkeypatch):
    from tripled_amd import native
    calls = []

    class Lib:
        def __getattr__(self, name):
            return lambda *args: calls.append(name) or 0

    monkeypatch.setattr(native, "load", lambda path=None: Lib())
    monkeypatch.setattr(native, "stream", lambda: None)
    return native, calls


def test_call_refuses_a_host_tensor(stub):
    native, calls = stub
    with pytest.raises(native.NativeLibraryError, match=r"needs device tensors \(got a cpu tensor\)"):
        native.call("td_pack_rgbx", torch.zeros(1, 3, 4, 4), 1, 4, 4, torch.zeros(1, 4, 4, 4))
    with pytest.raises(native.NativeLibraryError, match="needs device tensors"):
        native.call("td_photo_identity", None, [torch.zeros(4)], 1, 1, 4, 4, None, None, None)
    assert calls == []


def test_call_refuses_a_tensor_that_is_not_dense(stub, monkeypatch):
    native, calls = stub
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    x = torch.zeros(2, 8, 4, 4)
    with pytest.raises(native.NativeLibraryError, match="needs contiguous tensors"):
        native.call("td_pack_rgbx", x[:, ::2], 1, 4, 4, x)
    with pytest.raises(native.NativeLibraryError, match="needs contiguous tensors"):
        native.call("td_photo_identity", x, [x, x[:, ::2]], 1, 1, 4, 4, None, None, None)
    assert calls == []
    native.call("td_pack_rgbx", x, 1, 4, 4, x.contiguous(memory_format=torch.channels_last))      # both dense layouts pass
    assert calls == ["td_pack_rgbx"]


def test_call_refuses_a_wrong_argument_count_and_an_unknown_name(stub, monkeypatch):
    native, calls = stub
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(TypeError, match="td_pack_rgbx"):
        native.call("td_pack_rgbx", x, 1, 4, 4, x, 0)
    with pytest.raises(TypeError, match="td_pack_rgbx"):
        native.call("td_pack_rgbx", x, 1, 4, 4)
    with pytest.raises(KeyError):
        native.call("td_no_such_entry_point", x)
    with pytest.raises(TypeError, match="list of tensors"):      # a pointer array holds tensors, nothing else
        native.call("td_photo_identity", x, [x, None], 1, 1, 4, 4, None, None, None)
    with pytest.raises(TypeError, match="a tensor, None or a c_void_p"):
        native.call("td_pack_rgbx", x, 1, 4, 4, 12345)
    assert calls == []
