"""Driver of the call-trace test of tripled_amd.ops (tests/test_ops_calls_cpu.py) and of tools/gen_golden_ops_calls.py.

``record(patch)`` runs every op of ops.py forward and backward on CPU tensors against a stand-in library and returns, per case,
the C-ABI calls the op made (every argument described: see ``_Stub``) and the entry points ``native.check`` counted.  Nothing is
computed: the outputs are whatever ``torch.empty`` holds.  ``patch`` is ``monkeypatch.setattr`` (or ``pytest.MonkeyPatch().setattr``
in the tool), so every patch is undone by its owner.
"""
import collections
import ctypes
import json
import os
import socket

import torch
import torch.distributed as dist

GOLDEN_NAME = "ops_calls.json"
BF, F32, CL = torch.bfloat16, torch.float32, torch.channels_last


class _Stub:
    """Stands in for the ctypes handle: any ``td_*`` attribute is a function that checks its argument count against
    native.SIGNATURES, records ``[name, *described arguments]`` and returns a size (queries) or 0 (launches)."""

    def __init__(self, signatures, tensors):
        self.signatures, self.tensors, self.calls = signatures, tensors, []

    def _tensor(self, address):
        return self.tensors.get(address, "unknown") if address else None

    def _describe(self, a, slot):
        if a is None:
            return None
        if isinstance(a, ctypes.c_void_p):
            return self._tensor(a.value)
        if isinstance(a, ctypes.Array):
            if a._type_ is ctypes.c_void_p:
                return [self._tensor(v) for v in a]
            return list(a)
        if slot is ctypes.c_void_p and isinstance(a, int):
            return self._tensor(a)
        return a

    def __getattr__(self, name):
        if not name.startswith("td_"):
            raise AttributeError(name)
        slots = self.signatures[name][1]

        def fn(*args):
            assert len(args) == len(slots), "%s takes %d arguments, got %d" % (name, len(slots), len(args))
            self.calls.append([name] + [self._describe(a, s) for a, s in zip(args, slots)])
            if name.endswith(("_num_blocks", "_num_tasks", "_rows")):
                return 4
            return 64 if "workspace" in name else 0
        return fn


def install(patch):
    """Patch native / torch for a CPU run; returns (stub, ops, dispatch)."""
    import tripled_amd  # noqa: F401
    from tripled_amd import dispatch, native, ops
    tensors = {}
    stub = _Stub(native.SIGNATURES, tensors)
    data_ptr = torch.Tensor.data_ptr

    def recording_data_ptr(self):
        address = data_ptr(self)
        tensors[address] = [str(self.dtype), list(self.shape), list(self.stride())]
        return address

    patch(native, "load", lambda path=None: stub)
    patch(native, "require_device", lambda *tensors: None)
    patch(native, "stream", lambda: None)
    patch(torch.Tensor, "is_cuda", property(lambda self: True))
    patch(torch.Tensor, "data_ptr", recording_data_ptr)
    patch(dispatch, "hip_calls", collections.Counter())
    patch(dispatch, "fallbacks", collections.Counter())
    patch(ops, "WGRAD_GROUP", "node")
    return stub, ops, dispatch


def _act(c=64, n=2, h=4, w=6, dtype=BF, grad=True):
    return torch.zeros(n, c, h, w, dtype=dtype).contiguous(memory_format=CL).requires_grad_(grad)


def _par(*shape, dtype=F32, cl=False):
    t = torch.ones(*shape, dtype=dtype)
    if cl:
        t = t.contiguous(memory_format=CL)
    return t.requires_grad_(True)


def _bwd(out, nchw=False):
    """Back-propagate ones: in the output's own layout, or (``nchw``) as a planar gradient the node has to re-lay."""
    out.backward(torch.ones(out.shape, dtype=out.dtype) if nchw else torch.ones_like(out))


def _bn(c):
    return torch.nn.BatchNorm2d(c)


def _cases(ops, patch):
    """Yields (case name, thunk)."""
    tgt = torch.zeros(1, 3, 16, 32)
    srcs = [torch.zeros(1, 3, 16, 32), torch.zeros(1, 3, 16, 32)]
    invK = torch.eye(4).reshape(1, 4, 4)
    img8 = torch.zeros(1, 3, 8, 16)

    yield "pack_frames pack", lambda: ops.pack_frames(tgt, srcs, pack=True)
    yield "pack_frames lazy", lambda: ops.pack_frames(tgt, srcs, pack=False)
    yield "photo_identity tensors", lambda: ops.photo_identity(tgt, srcs)
    yield "photo_identity packed", lambda: ops.photo_identity(ops.pack_frames(tgt, srcs))
    yield "area_downsample", lambda: ops.area_downsample(tgt, 8, 16)
    yield "area_downsample same size", lambda: ops.area_downsample(tgt, 16, 32)

    def photo(idloss, noise, keep_warped, grad=True):
        def run():
            disp, P = torch.zeros(1, 1, 8, 16, requires_grad=grad), torch.zeros(2, 1, 3, 4, requires_grad=grad)
            fr = ops.pack_frames(tgt, srcs, pack=False)
            idl = ops.photo_identity(fr) if idloss else None
            nz = torch.zeros(2, 1, 16, 32) if noise else None
            loss, _, _ = ops.photometric_scale_loss(disp, P, fr, None, invK, idloss=idl, noise=nz, keep_warped=keep_warped)
            if grad:
                loss.backward()
        return run
    yield "photometric plain", photo(False, False, False)
    yield "photometric idloss noise warped", photo(True, True, True)
    yield "photometric idloss", photo(True, False, False)
    yield "photometric no grad", photo(False, True, False, grad=False)

    def frames_from_tensors():
        disp, P = torch.zeros(1, 1, 8, 16, requires_grad=True), torch.zeros(2, 1, 3, 4, requires_grad=True)
        ops.photometric_scale_loss(disp, P, tgt, srcs, invK)[0].backward()
    yield "photometric unpacked frames", frames_from_tensors

    def smooth(normalize):
        def run():
            disp = torch.zeros(1, 1, 8, 16, requires_grad=True)
            ops.smooth_loss(disp, img8, normalize=normalize, weight=0.5).backward()
        return run
    yield "smooth_loss normalize", smooth(True)
    yield "smooth_loss raw", smooth(False)

    for name, fn in (("maxpool5", ops.maxpool5), ("maxpool3s2", ops.maxpool3s2), ("reflpad1", ops.reflpad1),
                     ("up2_reflpad1", ops.up2_reflpad1)):
        for dtype in (BF, F32):
            for nchw in (False, True):
                yield ("%s %s%s" % (name, dtype, " planar grad" if nchw else ""),
                       lambda fn=fn, dtype=dtype, nchw=nchw: _bwd(fn(_act(dtype=dtype)), nchw))

    def crp(nchw):
        ws = [_par(64, 64, 1, 1, dtype=BF), _par(64, 64, 1, 1, dtype=BF, cl=True)]
        _bwd(ops.crp_block(_act(), ws), nchw)
    yield "crp_block", lambda: crp(False)
    yield "crp_block planar grad", lambda: crp(True)

    for nchw in (False, True):
        tag = " planar grad" if nchw else ""
        yield "join_channels" + tag, lambda nchw=nchw: _bwd(ops.join_channels(_act(), _act(8), _act(3)), nchw)
        yield "join_channels_up2" + tag, lambda nchw=nchw: _bwd(ops.join_channels_up2(_act(), _act(8, h=2, w=3), _act(3)), nchw)

    def bn(fn, dtype, residual, relu, running, groups, nchw=False, **kw):
        def run():
            x = _act(dtype=dtype)
            res = _act(dtype=dtype) if residual == "same" else _act(dtype=F32 if dtype is BF else BF) if residual else None
            rm, rv = (torch.zeros(groups * 64), torch.ones(groups * 64)) if running else (None, None)
            _bwd(fn(x, _par(64), _par(64), rm, rv, 0.1, 1e-5, residual=res, relu=relu, groups=groups, **kw), nchw)
        return run
    for dtype in (F32, BF):
        for residual in (None, "same"):
            for relu in (False, True):
                for running in (False, True):
                    for groups in (1, 2):
                        yield ("batchnorm_act %s res=%s relu=%d running=%d groups=%d" % (dtype, residual, relu, running, groups),
                               bn(ops.batchnorm_act, dtype, residual, relu, running, groups))
    yield "batchnorm_act residual of the other dtype, planar grad", bn(ops.batchnorm_act, BF, "other", True, True, 1, nchw=True)

    def conv_bn(stride, residual, relu, groups=1, nchw=False):
        def run():
            res = _act(h=(4 - 1) // stride + 1, w=(6 - 1) // stride + 1) if residual else None
            y = ops.conv1x1_bn_act(_act(), _par(64, 64, 1, 1, dtype=BF), _par(64), _par(64), torch.zeros(groups * 64),
                                   torch.ones(groups * 64), 0.1, 1e-5, residual=res, relu=relu, groups=groups, stride=stride)
            _bwd(y, nchw)
        return run
    for stride in (1, 2):
        for residual in (False, True):
            for relu in (False, True):
                yield "conv1x1_bn_act stride=%d res=%d relu=%d" % (stride, residual, relu), conv_bn(stride, residual, relu)
    yield "conv1x1_bn_act groups=2 planar grad", conv_bn(1, True, True, groups=2, nchw=True)

    def no_running_stats():
        y = ops.conv1x1_bn_act(_act(grad=False), _par(64, 64, 1, 1, dtype=BF), _par(64), _par(64), None, None, 0.1, 1e-5)
        _bwd(y)
    yield "conv1x1_bn_act no running stats, no data gradient", no_running_stats

    def bias_act(act, bias, nchw=False):
        def run():
            b = _par(8, dtype=bias) if bias is not None else None
            _bwd(ops.conv_bias_act(_act(), _par(8, 64, 3, 3, dtype=BF, cl=True), b, act), nchw)
        return run
    for act in (None, "elu", "leaky_relu"):
        for bias in (None, F32, BF):
            yield "conv_bias_act %s bias=%s" % (act, bias), bias_act(act, bias)
    yield "conv_bias_act elu planar grad", bias_act("elu", F32, nchw=True)

    def bottleneck(cout, stride, groups=1, nchw=False):
        def run():
            down = cout != 64 or stride != 1
            wd, bnd = (_par(cout, 64, 1, 1, dtype=BF), _bn(cout)) if down else (None, None)
            y = ops.bottleneck(_act(), _par(64, 64, 1, 1, dtype=BF), _bn(64), _par(64, 64, 3, 3, dtype=BF, cl=True), _bn(64),
                               _par(cout, 64, 1, 1, dtype=BF), _bn(cout), wd, bnd, groups=groups, stride=stride)
            _bwd(y, nchw)
        return run
    for mode in ("node", "off", "step"):
        def with_mode(thunk, mode=mode):
            def run():
                patch(ops, "WGRAD_GROUP", mode)
                try:
                    if mode == "step":
                        with ops.deferred_wgrads():
                            thunk()
                    else:
                        thunk()
                finally:
                    patch(ops, "WGRAD_GROUP", "node")
            return run
        yield "bottleneck identity wgrad=%s" % mode, with_mode(bottleneck(64, 1))
        yield "bottleneck down-sample stride 1 wgrad=%s" % mode, with_mode(bottleneck(128, 1))
        yield "bottleneck down-sample stride 2 wgrad=%s" % mode, with_mode(bottleneck(128, 2))
        yield "crp_block wgrad=%s" % mode, with_mode(lambda: crp(False))

        def wgrads():
            w = _par(64, 64, 1, 1, dtype=BF)
            prob = (_act(grad=False), _act(grad=False), w, 48, 64, 64, 4, 6, 1)
            outs = [ops.conv1x1_wgrad(*prob)]
            with ops.wgrad_group():
                outs.append(ops.conv1x1_wgrad(*prob))
            with ops.deferred_wgrads():      # the same leaf weight twice: first use stores .grad, the second adds
                with ops.wgrad_group():
                    outs += [ops.conv1x1_wgrad(*prob), ops.conv1x1_wgrad(*prob)]
            return [o is None for o in outs], w.grad is None
        yield "conv1x1_wgrad wgrad=%s" % mode, with_mode(wgrads)
    yield "bottleneck groups=2 planar grad", bottleneck(128, 2, groups=2, nchw=True)

    yield "conv3x3_wgrad", lambda: ops.conv3x3_wgrad(_act(grad=False), _act(grad=False), _par(64, 64, 3, 3, dtype=BF, cl=True), pad=1)

    def sync_bn(dtype, residual, relu, running, groups=1, nchw=False):
        inner = bn(lambda *a, **kw: ops.sync_batchnorm_act(*a, process_group=dist.group.WORLD, **kw), dtype, residual, relu, running,
                   groups, nchw)

        def run():
            own = not dist.is_initialized()
            if own:
                s = socket.socket()
                s.bind(("127.0.0.1", 0))
                port = s.getsockname()[1]
                s.close()
                dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
            try:
                inner()
            finally:
                if own:
                    dist.destroy_process_group()
        return run
    yield "sync_batchnorm_act bf16 res relu running", sync_bn(BF, "same", True, True)
    yield "sync_batchnorm_act f32 res", sync_bn(F32, "same", False, False, groups=2)
    yield "sync_batchnorm_act bf16 relu planar grad", sync_bn(BF, None, True, True, nchw=True)
    yield "sync_batchnorm_act residual of the other dtype", sync_bn(BF, "other", True, False)

    yield "edge_weights", lambda: ops.edge_weights(img8, 1.5, [1, 2, 3, 4, 5, 6])
    for dtype in (BF, F32):
        yield ("feature_regularization %s" % dtype,
               lambda dtype=dtype: ops.feature_regularization(_act(dtype=dtype), torch.zeros(2, 3, 4, 6), 1e-3, 1e-3).backward())

    def recon():
        pred = torch.zeros(1, 3, 8, 16, dtype=BF).contiguous(memory_format=CL).requires_grad_(True)
        ops.masked_reconstruction_sum(pred, img8, torch.zeros(1, 8, 16)).backward()
    yield "masked_reconstruction_sum", recon

    def featwarp(n_src, dtype):
        def run():
            disp, P = torch.zeros(1, 1, 8, 16, requires_grad=True), torch.zeros(n_src, 1, 3, 4, requires_grad=True)
            feats = [_act(n=1, h=4, w=8, dtype=dtype) for _ in range(n_src + 1)]
            ops.feature_warp_min_loss(feats[0], feats[1:], disp, P, invK, 0.1, 100.0)[0].backward()
        return run
    yield "feature_warp_min_loss 2 sources bf16", featwarp(2, BF)
    yield "feature_warp_min_loss 1 source f32", featwarp(1, F32)

    def l1map(dtype, cl):
        def run():
            pred = torch.zeros(1, 3, 8, 16, dtype=dtype)
            pred = (pred.contiguous(memory_format=CL) if cl else pred).requires_grad_(True)
            ops.robust_l1_map(pred, img8, weight=0.25).mean().backward()
        return run
    yield "robust_l1_map planar f32", l1map(F32, False)
    yield "robust_l1_map channels-last bf16", l1map(BF, True)

    yield "rgb2lab", lambda: ops.rgb2lab(img8)

    def pose(both):
        def run():
            a, t = torch.zeros(2, 1, 3, requires_grad=True), torch.zeros(2, 1, 3, requires_grad=True)
            T, P = ops.pose_transforms(a, t, invK, [True, False])
            (P.sum() + T.sum() if both else P.sum()).backward()
        return run
    yield "pose_transforms P and T", pose(True)
    yield "pose_transforms P only", pose(False)

    yield "color_jitter_expand", lambda: ops.color_jitter_expand(torch.zeros(2, 3, 8, 16, dtype=torch.uint8), torch.zeros(2, 9))
    yield "quantize_fp8 channels-last bf16", lambda: ops.quantize_fp8(_act(grad=False))
    yield "quantize_fp8 planar f32", lambda: ops.quantize_fp8(torch.zeros(2, 64, 4, 6))


def record(patch):
    """[[case, calls, dispatch snapshot], ...] of every case, each from fresh counters."""
    stub, ops, dispatch = install(patch)
    trace = []
    for name, thunk in _cases(ops, patch):
        del stub.calls[:]
        dispatch.reset()
        thunk()
        trace.append([name, list(stub.calls), dispatch.snapshot()])
    return trace


def dumps(trace):
    """One case per line, no spaces: compact, and a changed case shows as one changed line."""
    return "[\n" + ",\n".join(json.dumps(case, separators=(",", ":"), sort_keys=True) for case in trace) + "\n]\n"


def golden_path(root):
    return os.path.join(root, "tests", "golden", GOLDEN_NAME)
