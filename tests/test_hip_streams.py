"""tripled_amd.streams: the three independent chains of the TripleD step on concurrent HIP streams give the step the serial
order gives -- the forward losses to fp32 rounding of MIOpen's run-to-run summation order (the chains share no buffer), the
gradients within the run-to-run spread MIOpen's order-dependent weight-gradient solvers have anyway."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _step(fork):
    import tripled_amd  # noqa: F401
    from tripled_amd import streams
    from mono.datasets import synthetic_batch
    from mono.model import MONO
    from tests.test_hip_model_step import _opt
    name = "mono_fm_joint_inpaint_disentangle"
    B, H, W = 2, 96, 160
    torch.manual_seed(11)
    model = MONO.module_dict[name](_opt(name, B, H, W)).cuda().train()
    model.DepthDecoder.do.eval()
    model.set_noise_source(lambda shape, device: torch.zeros(shape, device=device))
    batch = {k: v.cuda() for k, v in synthetic_batch(B, H, W, seed=3).items()}
    old = streams.ENABLED
    streams.ENABLED = fork
    try:
        _, losses = model(batch)
        sum(v.mean() for v in losses.values()).backward()
        torch.cuda.synchronize()
    finally:
        streams.ENABLED = old
    grads = torch.cat([p.grad.float().flatten() for p in model.parameters() if p.grad is not None])
    return {str(k): v.detach().float().mean().item() for k, v in losses.items()}, grads


def test_forked_step_equals_serial_step():
    l_fork, g_fork = _step(True)
    l_ser, g_ser = _step(False)
    l_ser2, g_ser2 = _step(False)
    assert l_fork.keys() == l_ser.keys()
    for k in l_ser:
        # forward: the chains share no buffer, so the values agree to the last bits -- not always ALL bits: MIOpen's fp32
        # forward solvers on these small maps sum in an order that varies from run to run (1e-7 relative, serial runs too)
        spread = abs(l_ser2[k] - l_ser[k])
        assert abs(l_fork[k] - l_ser[k]) <= 4 * spread + 2e-6 * abs(l_ser[k]), (k, l_fork[k], l_ser[k], l_ser2[k])
    rel = lambda a, b: ((a - b).norm() / b.norm().clamp_min(1e-12)).item()
    noise = rel(g_ser2, g_ser)                   # serial against serial: MIOpen's own run-to-run spread
    assert rel(g_fork, g_ser) <= 1.25 * noise + 0.02, (rel(g_fork, g_ser), noise)
    assert torch.isfinite(g_fork).all()


def test_branch_orders_the_streams_and_marks_the_tensors():
    import tripled_amd  # noqa: F401
    from tripled_amd import streams
    dev = torch.device("cuda", 0)
    a = torch.full((1 << 22,), 2.0, device=dev)
    with streams.Branch(dev, 0) as b:
        assert torch.cuda.current_stream() == b.stream and b.stream != torch.cuda.default_stream()
        out = {"x": [a * 3.0, (a + 1.0,)]}
    b.join(out)
    assert torch.cuda.current_stream() != b.stream
    assert float((out["x"][0] + out["x"][1][0]).sum()) == (6.0 + 3.0) * (1 << 22)
    assert streams.side_stream(dev, 0) is b.stream and streams.side_stream(dev, 1) is not b.stream


def test_a_branch_never_lands_on_the_current_stream():
    """torch.cuda.Stream() cycles through a pool of 32 HIP streams: a caller-side stream created later can alias a cached side
    stream.  Branch must then move to another stream (a fork onto the current stream is a self-wait and no branch at all;
    found while chasing the segfault of round 4's full suite) -- checked eagerly here, inside a capture
    by the next test."""
    import tripled_amd  # noqa: F401
    from tripled_amd import streams
    dev = torch.device("cuda", 0)
    first = streams.Branch(dev, 0).stream
    seen = set()
    for _ in range(40):                       # more than one round of the pool: every pooled stream is "current" once
        cur = torch.cuda.Stream()
        seen.add(int(cur.cuda_stream))
        with torch.cuda.stream(cur):
            b0, b1 = streams.Branch(dev, 0), streams.Branch(dev, 1)
            ids = {int(cur.cuda_stream), int(b0.stream.cuda_stream), int(b1.stream.cuda_stream)}
            assert len(ids) == 3 and 0 not in ids
    assert int(first.cuda_stream) in seen     # the aliasing case did occur in the loop


_ALIASED_CAPTURE = r"""
import torch
import tripled_amd
from tripled_amd import streams
assert streams.ENABLED
dev = torch.device("cuda", 0)
s0 = streams.Branch(dev, 0).stream                    # the cache takes a pooled stream ...
cap = None
for _ in range(80):                                   # ... and the pool comes round to it: THIS capture stream is that stream
    c = torch.cuda.Stream()
    if int(c.cuda_stream) == int(s0.cuda_stream):
        cap = c
        break
assert cap is not None, "the pool never handed the cached side stream out again"
x = torch.ones(1 << 20, device=dev)
g = torch.cuda.CUDAGraph()
torch.cuda.synchronize()
with torch.cuda.graph(g, stream=cap):
    with streams.Branch(dev, 0) as b0:
        y = x * 2.0
    with streams.Branch(dev, 1) as b1:
        w = x * 3.0
    z = x + 1.0
    ids = {int(cap.cuda_stream), int(b0.stream.cuda_stream), int(b1.stream.cuda_stream)}
    b1.join(w)
    b0.join(y)
    out = y + z + w
assert len(ids) == 3 and 0 not in ids, ids
for _ in range(3):
    x.add_(1.0)
    g.replay()
torch.cuda.synchronize()
assert float(out.sum()) == (2 * 4.0 + 5.0 + 3 * 4.0) * (1 << 20), float(out.sum())
print("ALIASED-CAPTURE-OK")
"""


def test_a_forked_capture_on_a_stream_that_aliases_the_cached_side_stream_replays():
    """The aliasing case built deterministically: the capture stream IS the pooled stream the side-stream cache took earlier.  Branch has to move to other streams, the captured graph has three distinct branches and replays.  In a fresh
    process, like every capture of a forked step in this suite (tests/conftest.py): a fault in hipGraphLaunch takes the
    process down, and the long pytest process is not the place to find out."""
    env = dict(os.environ)
    env.pop("TD_BRANCH_STREAMS", None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", _ALIASED_CAPTURE], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ALIASED-CAPTURE-OK" in out.stdout, (out.returncode, out.stdout[-500:], out.stderr[-2000:])


def test_bench_replays_the_forked_step_from_a_hip_graph():
    """The product path: bench.py in a fresh process captures the cfg_kitti_tripleD step with the forks on (three parallel
    branches in the HIP graph, forward and backward), replays it through both entries (TrainStep and Runner.run) and reports
    a finite, moving loss with zero ATen fallbacks."""
    env = dict(os.environ)
    env.pop("TD_BRANCH_STREAMS", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2", "--full", "--no-cpu-baseline",
                          "--no-roofline", "--miopen-find", "off"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    c = line["config"]
    assert c["branch_streams"] is True and c["hip_graph"] and c["valid"] and c["fallbacks"] == 0, c
    assert line["runner_entry"]["ms_per_step"] > 0, line["runner_entry"]
