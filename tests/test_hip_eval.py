"""csrc/td_eval.hip on the device (through tripled_amd.evaluate): the exact masked median against np.median bit for bit, the
batched KITTI protocol against oracle.metrics.eval_single image by image, then DepthEvaluator and the evaluation hook against the
one-frame-at-a-time host path.  Bounds: tests/eval_util.py (counts exact; scale and the error metrics within
max(10 x the float32 host path's own distance from float64, 1e-5 relative); a1..a3 within the pixels that lie on a threshold)."""
import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import evaluate, infer
from tests import eval_util as U
from tests.infer_util import ROOT, build_model

pytestmark = pytest.mark.gpu

CASES = {"mixed": (U.MIXED_SIZES, 16, 24, 3), "kitti": (U.KITTI_SIZES[:2], 192, 640, 5)}
_cache = {}


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_on_the_device():
    """The cached model, cases and workspaces go when the module is done: the tests after it in the same process (graph capture
    of the whole training step among them) find the device as they would without this file."""
    yield
    import gc
    _cache.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- 1. the select ---------------------------------------------------------------------------------------------------------------

def _median_rows(n, seed):
    """[rows, n] float32; an entry <= 0 is absent."""
    g = np.random.default_rng(seed)
    spread = np.exp(g.uniform(np.log(1e-3), np.log(80.0), n)).astype(np.float32)            # 1e-3 .. 80
    few = g.choice(np.float32([0.75, 1.5, 1.5000001, 20.0, 79.5]), n).astype(np.float32)     # 5 distinct values
    two = np.where(np.arange(n) < n // 2, np.float32(2.0), np.float32(3.0)).astype(np.float32)
    g.shuffle(two)                                                                         # middle ranks straddle 2 | 3
    low_bits = (np.float32(1.0).view(np.uint32) + g.integers(0, 8, n).astype(np.uint32)).view(np.float32)
    rows = [spread.copy(), spread.copy(), few.copy(), few.copy(), two, low_bits, np.full(n, 3.25, np.float32)]
    rows[1][g.integers(0, n)] = 0.0                                                        # the other parity of the count
    rows[3][g.integers(0, n)] = -1.0
    sparse = np.where(g.random(n) < 0.3, spread, np.float32(0.0)).astype(np.float32)        # most entries absent
    one = np.zeros(n, np.float32)
    one[g.integers(0, n)] = 7.5                                                            # count 1
    pair = np.zeros(n, np.float32)
    pair[[0, n - 1]] = [1e-3, 80.0]                                                        # count 2
    none = -np.abs(spread)
    none[::2] = 0.0                                                                        # count 0
    return np.stack(rows + [sparse, one, pair, none], 0)


@pytest.mark.parametrize("n", [7, 1000, 300000])
def test_masked_median_is_numpys(n):
    vals = _median_rows(n, n)
    med, cnt = evaluate.masked_median_hip(torch.from_numpy(vals).to(_dev()))
    med, cnt = med.cpu().numpy(), cnt.cpu().numpy()
    assert med.dtype == np.float32 and cnt.dtype == np.int32
    parities = set()
    for r, row in enumerate(vals):
        present = row[row > 0]
        assert cnt[r] == present.size, (r, cnt[r], present.size)
        if present.size == 0:
            assert np.isnan(med[r])
            continue
        want = np.median(present)
        assert want.dtype == np.float32
        assert med[r].view(np.uint32) == want.view(np.uint32), "row %d (count %d): %r, numpy %r" % (r, present.size, med[r], want)
        parities.add(present.size % 2)
    assert parities == {0, 1} and set(cnt[-3:].tolist()) == {0, 1, 2}
    again, _ = evaluate.masked_median_hip(torch.from_numpy(vals).to(_dev()))
    assert np.array_equal(again.cpu().numpy().view(np.uint32), med.view(np.uint32))


# ---- 2. the protocol -----------------------------------------------------------------------------------------------------------

def _case(name, dtype):
    """(disp on the device, ground truths, {stereo: references}); computed once per case and dtype."""
    key = (name, dtype)
    if key not in _cache:
        sizes, h, w, seed = CASES[name]
        disp, gts = U.make_case(seed, sizes, h, w, dtype)
        refs = {s: [U.Reference(U.scaled_disparity(disp[i]), gts[i], s) for i in range(len(sizes))] for s in (False, True)}
        _cache[key] = (disp, gts, refs)
    return _cache[key]


@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", sorted(CASES))
def test_eval_kernel_against_oracle(name, dtype, stereo):
    disp, gts, refs = _case(name, dtype)
    gt, sizes, crops = evaluate.pad_ground_truth(gts, _dev())
    rows, counts = evaluate.evaluate_disparity_hip(disp.to(_dev()), gt, sizes, crops, stereo_scale=stereo, affine=U.AFFINE)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (len(gts), 8) and counts.dtype == torch.int32
    U.check_rows(rows.cpu().numpy(), counts.cpu().numpy(), refs[stereo], "kernel %s %s stereo %d" % (name, dtype, stereo))
    # the torch statements on the device say the same
    trows, tcounts = evaluate.evaluate_disparity_torch(disp.to(_dev()), gts, stereo_scale=stereo, affine=U.AFFINE)
    U.check_rows(trows.cpu().numpy(), tcounts.cpu().numpy(), refs[stereo], "torch on device %s %s stereo %d" % (name, dtype, stereo))


@pytest.mark.parametrize("name", sorted(CASES))
def test_eval_kernel_repeats_bit_for_bit(name):
    disp, gts, _ = _case(name, torch.float32)
    gt, sizes, crops = evaluate.pad_ground_truth(gts, _dev())
    d = disp.to(_dev())
    ws = evaluate.eval_workspace(len(gts), gt.shape[1], gt.shape[2], _dev())
    first = evaluate.evaluate_disparity_hip(d, gt, sizes, crops, workspace=ws)
    second = evaluate.evaluate_disparity_hip(d, gt, sizes, crops, workspace=ws)                  # the used workspace again
    third = evaluate.evaluate_disparity_hip(d, gt, sizes, crops)
    for other in (second, third):
        assert torch.equal(first[0].view(torch.int32), other[0].view(torch.int32)) and torch.equal(first[1], other[1])


def test_empty_frame_gives_nan_row_and_leaves_its_neighbours():
    disp, gts, _ = _case("mixed", torch.float32)
    gt, sizes, crops = evaluate.pad_ground_truth(gts, _dev())
    want, wcounts = evaluate.evaluate_disparity_hip(disp.to(_dev()), gt, sizes, crops)
    gt2 = gt.clone()
    gt2[1] = 0
    rows, counts = evaluate.evaluate_disparity_hip(disp.to(_dev()), gt2, sizes, crops)
    assert int(counts[1]) == 0 and bool(torch.isnan(rows[1]).all())
    assert torch.equal(rows[[0, 2]], want[[0, 2]]) and torch.equal(counts[[0, 2]], wcounts[[0, 2]])


def test_single_pixel_mask():
    disp, gts, _ = _case("mixed", torch.float32)
    one = np.zeros_like(gts[0])
    one[20, 30] = 12.5
    gt, sizes, crops = evaluate.pad_ground_truth([one, gts[1], gts[2]], _dev())
    # (stereo scaling: with the median ratio a single pixel's errors are exactly 0 and so is their bound)
    rows, counts = evaluate.evaluate_disparity_hip(disp.to(_dev()), gt, sizes, crops, stereo_scale=True, affine=U.AFFINE)
    ref = U.Reference(U.scaled_disparity(disp[0]), one, True)
    assert ref.N == 1
    U.check_rows(rows.cpu().numpy()[:1], counts.cpu().numpy()[:1], [ref], "one pixel")


def test_padding_never_enters():
    disp, gts, _ = _case("mixed", torch.float32)
    gt, sizes, crops = evaluate.pad_ground_truth(gts, _dev())
    want = evaluate.evaluate_disparity_hip(disp.to(_dev()), gt, sizes, crops)
    filled = torch.full_like(gt, 10.0)
    for i, (h, w) in enumerate(U.MIXED_SIZES):
        filled[i, :h, :w] = gt[i, :h, :w]
    assert int((filled != gt).sum()) > 0
    got = evaluate.evaluate_disparity_hip(disp.to(_dev()), filled, sizes, crops)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])


# ---- 3. the evaluator ----------------------------------------------------------------------------------------------------------

def _model():
    if "model" not in _cache:
        _cache["model"] = build_model("cfg_kitti_fm", 32, 64).to(_dev()).eval()
    return _cache["model"]


def _host_loop(model, data, stereo=False):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("eval_depth_script", os.path.join(ROOT, "scripts", "eval_depth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.evaluate(model, data, stereo, _dev())


@pytest.mark.parametrize("wire", ["float32", "uint8"])
def test_evaluator_against_the_host_loop(wire):
    model = _model()
    floats = U.ListDataset(7, 5, 64, 128, U.MIXED_SIZES)
    data = U.ListDataset(7, 5, 64, 128, U.MIXED_SIZES, wire=wire)
    refs = U.frame_references(model, floats, _dev(), False)
    host_mean, host_scales = _host_loop(model, floats)
    model.train()
    mean, scales = evaluate.DepthEvaluator(model, _dev(), batch_size=2).evaluate(data)
    assert model.training and next(model.parameters()).device == _dev()
    model.eval()
    U.check_mean(mean, scales, refs, "evaluator fp32 %s" % wire, want=host_mean, want_scales=host_scales)


def test_evaluator_with_flip_post_processing():
    from mono.core.evaluation import disp_to_depth  # noqa: F401
    model = _model()
    data = U.ListDataset(7, 5, 64, 128, U.MIXED_SIZES)
    disps = []
    with torch.no_grad():
        for i in range(5):
            x = data[i][("color", 0, 0)][None].to(_dev())
            d = model(infer.network_inputs(torch.cat([x, x.flip(3)], 0)))[("disp", 0, 0)]
            disps.append(infer.postprocess_torch(d, d.shape[2], d.shape[3], paired=True)[0][0])
    refs = U.frame_references(None, data, _dev(), False, disps=disps)
    mean, scales = evaluate.DepthEvaluator(model, _dev(), batch_size=2, post_process=True).evaluate(data)
    assert not model.training
    U.check_mean(mean, scales, refs, "evaluator fp32 flip")


def test_evaluator_bf16_runs_the_folded_copy():
    model = _model()
    data = U.ListDataset(7, 5, 64, 128, U.MIXED_SIZES)
    ev = evaluate.DepthEvaluator(model, _dev(), batch_size=2, precision="bf16")
    net, _ = infer.eval_network(model, _dev(), "bf16")
    assert net is not model and infer.count_batchnorms(net.DepthEncoder) == 0
    mean, scales = ev.evaluate(data)
    assert scales.shape == (5,) and np.isfinite(scales).all() and all(np.isfinite(mean[k]) for k in evaluate.METRICS)
    assert next(model.parameters()).dtype == torch.float32 and not model.training
    assert infer.count_batchnorms(model.DepthEncoder) > 0


# ---- 4. the hook ---------------------------------------------------------------------------------------------------------------

class _LogBuffer:
    def __init__(self):
        self.output, self.ready = {}, False


class _FakeRunner:
    def __init__(self, model):
        self.model, self.log_buffer, self.epoch, self.rank, self.world_size = model, _LogBuffer(), 0, 0, 1


def test_hook_validates_on_device():
    from mmcv import Config
    from mono.core.evaluation import NonDistEvalHook
    from mono.datasets.synthetic import SyntheticTripletDataset
    model = _model()
    data = SyntheticTripletDataset(5, 64, 128, frame_ids=[0], with_gt=True)
    out = {}
    for on_device in (False, True):
        cfg = Config(dict(data=dict(stereo_scale=False), validate_interval=1, work_dir="."))
        if on_device:
            cfg["validate_on_device"], cfg["validate_batch_size"] = True, 2
        runner = _FakeRunner(model)
        NonDistEvalHook(data, cfg).after_train_epoch(runner)
        assert runner.log_buffer.ready
        out[on_device] = dict(runner.log_buffer.output)
    assert set(out[True]) == set(out[False]) == set(evaluate.METRICS) | {"scale mean", "scale std"}
    refs = U.frame_references(model, data, _dev(), False)
    mean = {k: out[True][k] for k in evaluate.METRICS}
    scales = [r.row[7] for r in refs]
    U.check_mean(mean, scales, refs, "hook on device")
    bound = float(np.mean([r.bound[7] for r in refs]))
    assert abs(out[True]["scale mean"] - out[False]["scale mean"]) <= bound
