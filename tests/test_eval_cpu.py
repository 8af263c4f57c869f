"""tripled_amd.evaluate on the host: the torch statements of the batched KITTI protocol against oracle.metrics.eval_single image
by image, the Garg crops, DepthEvaluator(device='cpu') against the per-frame host path, and the argument checks of the C-ABI
entries of csrc/td_eval.hip (no GPU needed: nothing is launched on a bad argument).  Bounds: tests/eval_util.py."""
import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import evaluate, native
from tests import eval_util as U
from tests.infer_util import build_model


@pytest.mark.parametrize("stereo", [False, True])
def test_torch_statements_against_oracle(stereo):
    disp, gts = U.make_case(3, U.MIXED_SIZES, 16, 24)
    rows, counts = evaluate.evaluate_disparity_torch(disp, gts, stereo_scale=stereo, affine=U.AFFINE)
    assert tuple(rows.shape) == (3, 8) and rows.dtype == torch.float32 and counts.dtype == torch.int32
    refs = [U.Reference(U.scaled_disparity(disp[i]), gts[i], stereo) for i in range(3)]
    assert all(0.2 < r.N / (0.54 * g.size) < 0.4 for r, g in zip(refs, gts))          # sparse: about 30 % of the crop
    U.check_rows(rows.numpy(), counts.numpy(), refs, "torch stereo %d" % stereo)
    default = evaluate.evaluate_disparity_torch(disp[:, None], gts, stereo_scale=stereo)          # [B,1,h,w], default affine
    assert torch.equal(default[0], rows) and torch.equal(default[1], counts)


def test_empty_mask_gives_nan_row():
    disp, gts = U.make_case(4, U.MIXED_SIZES, 16, 24)
    want, _ = evaluate.evaluate_disparity_torch(disp, gts)
    gts[1] = np.zeros_like(gts[1])
    rows, counts = evaluate.evaluate_disparity_torch(disp, gts)
    assert counts.tolist()[1] == 0 and bool(torch.isnan(rows[1]).all())
    assert torch.equal(rows[[0, 2]], want[[0, 2]])


def test_median_is_numpys():
    g = np.random.default_rng(0)
    for n in (1, 2, 7, 8, 1001):
        v = g.choice(np.float32([0.5, 1.25, 3.0, 3.0000002, 80.0]), n).astype(np.float32)
        assert float(evaluate.median_torch(torch.from_numpy(v))) == float(np.median(v))


def test_crops_equal_the_oracles_integers():
    gts = [np.zeros(s, np.float32) for s in U.KITTI_SIZES]
    gt, sizes, crops = evaluate.pad_ground_truth(gts, "cpu")
    assert tuple(gt.shape) == (4, 376, 1242) and gt.dtype == torch.float32
    assert sizes.dtype == torch.int32 and sizes.tolist() == [list(s) for s in U.KITTI_SIZES]
    for (gt_h, gt_w), crop in zip(U.KITTI_SIZES, crops.numpy()):
        want = np.array([0.40810811 * gt_h, 0.99189189 * gt_h, 0.03594771 * gt_w, 0.96405229 * gt_w]).astype(np.int32)
        assert crop.dtype == np.int32 and np.array_equal(crop, want)
    assert crops[0].tolist() == [153, 371, 44, 1197]


def test_padding_holds_the_images_top_left():
    gts = [np.full(s, i + 1.0, np.float32) for i, s in enumerate(U.MIXED_SIZES)]
    gt, _, _ = evaluate.pad_ground_truth(gts, "cpu")
    for i, (h, w) in enumerate(U.MIXED_SIZES):
        assert float(gt[i, :h, :w].min()) == i + 1.0 and float(gt[i].sum()) == (i + 1.0) * h * w


@pytest.mark.parametrize("wire", ["float32", "uint8"])
@pytest.mark.parametrize("post_process", [False, True])
def test_evaluator_on_the_host(post_process, wire):
    from mono.core.evaluation import disp_to_depth, evaluate_disparity
    from tripled_amd import infer
    model = build_model("cfg_kitti_fm", 32, 64).eval()
    data = U.ListDataset(7, 5, 64, 128, U.MIXED_SIZES, wire=wire)
    floats = U.ListDataset(7, 5, 64, 128, U.MIXED_SIZES)
    model.train()
    ev = evaluate.DepthEvaluator(model, "cpu", batch_size=2, post_process=post_process)
    mean, scales = ev.evaluate(data)
    assert model.training and next(model.parameters()).device.type == "cpu"
    assert set(mean) == set(evaluate.METRICS) and scales.shape == (5,)
    model.eval()
    disps = []
    with torch.no_grad():
        for i in range(5):
            x = floats[i][("color", 0, 0)][None]
            if post_process:
                x = torch.cat([x, x.flip(3)], 0)
            d = model(infer.network_inputs(x))[("disp", 0, 0)]
            disps.append(infer.postprocess_torch(d, d.shape[2], d.shape[3], paired=True)[0][0] if post_process else d[0, 0])
    host = [evaluate_disparity(disp_to_depth(d, 0.1, 100)[0].numpy(), floats[i]["gt_depth"]) for i, d in enumerate(disps)]
    refs = U.frame_references(None, floats, "cpu", False, disps=disps)
    for r, ref in zip(host, refs):                       # evaluate_disparity and the oracle are the same statements
        assert [r[k] for k in U.NAMES] == ref.row.tolist()
    U.check_mean(mean, scales, refs, "host evaluator post_process %d %s" % (post_process, wire))


def test_evaluator_names_the_frame_with_an_empty_mask():
    model = build_model("cfg_kitti_fm", 32, 64).eval()
    data = U.ListDataset(6, 3, 64, 128, U.MIXED_SIZES)
    data.samples[2]["gt_depth"] = np.zeros((24, 40), np.float32)
    with pytest.raises(ValueError, match="frame 2"):
        evaluate.DepthEvaluator(model, "cpu", batch_size=2).evaluate(data)
    with pytest.raises(ValueError):
        evaluate.DepthEvaluator(model, "cpu", precision="bf16")


def test_entry_points_reject_bad_arguments_without_gpu():
    lib = native.load()
    assert lib.td_eval_depth(None, 0, 1, 8, 8, 9.99, 0.01, None, 8, 8, None, None, 1e-3, 80.0, 0, None, 0, None, None, None) == -1
    assert lib.td_masked_median(None, 1, 8, None, 0, None, None, None) == -1
    assert lib.td_eval_depth_workspace_bytes(0, 8, 8) == 0 and lib.td_masked_median_workspace_bytes(0) == 0
    small, big = lib.td_eval_depth_workspace_bytes(1, 37, 61), lib.td_eval_depth_workspace_bytes(12, 376, 1242)
    assert small >= 37 * 61 * 4 and big >= 12 * 376 * 1242 * 4 and big > small
    assert lib.td_masked_median_workspace_bytes(3) > 0


def test_kernel_wrappers_refuse_host_tensors():
    disp, gts = U.make_case(3, U.MIXED_SIZES, 16, 24)
    gt, sizes, crops = evaluate.pad_ground_truth(gts, "cpu")
    with pytest.raises(native.NativeLibraryError):
        evaluate.evaluate_disparity_hip(disp, gt, sizes, crops)
    with pytest.raises(native.NativeLibraryError):
        evaluate.masked_median_hip(torch.rand(2, 7))


def test_require_device():
    native.require_device()
    with pytest.raises(native.NativeLibraryError, match=r"libtripled_hip needs device tensors \(got a cpu tensor\)"):
        native.require_device(torch.zeros(1))
    with pytest.raises(native.NativeLibraryError, match=r"libtripled_hip needs device tensors \(got a cpu tensor\)"):
        native.ptr(torch.zeros(1))


@pytest.mark.parametrize("wire", ["float32", "uint8"])
def test_collate_validation_on_the_host(wire):
    from mono.datasets import SyntheticTripletDataset, collate_validation
    ds = SyntheticTripletDataset(2, 16, 24, with_gt=True, wire=wire)
    samples = [ds[0], ds[1]]
    batch = collate_validation(samples, "cpu")
    assert "gt_depth" in samples[0] and "gt_depth" not in batch and "aug" not in batch
    expanded = set()
    if wire == "uint8":
        assert "aug" in samples[0]
        for f in ds.frame_ids:
            u8 = torch.stack([s[("color_u8", f)] for s in samples], 0)
            assert u8.dtype == torch.uint8 and ("color_u8", f) not in batch
            assert batch[("color", f, 0)] is batch[("color_aug", f, 0)] and torch.equal(batch[("color", f, 0)], u8.float() / 255)
            expanded |= {("color", f, 0), ("color_aug", f, 0)}
    others = [k for k in samples[0] if k not in ("gt_depth", "aug") and not (isinstance(k, tuple) and k[0] == "color_u8")]
    assert set(batch) == set(others) | expanded and len(others) >= 3
    for k in others:
        assert batch[k].dtype == torch.float32 and batch[k].shape[0] == 2
        assert torch.equal(batch[k], torch.stack([torch.as_tensor(s[k]) for s in samples], 0).float())


def test_collate_validation_refuses_raw_frames_on_the_host():
    from mono.datasets import SyntheticTripletDataset, collate_validation
    ds = SyntheticTripletDataset(1, 16, 24, frame_ids=(0,), with_gt=True, wire="raw_u8", raw_sizes=[(20, 30)])
    assert ("raw_u8", 0) in ds[0]
    with pytest.raises(native.NativeLibraryError, match="raw_u8"):
        collate_validation([ds[0]], "cpu")
