"""tripled_amd.infer on the host: the three host statements against the reference's recorded outputs (tests/golden/infer.npz,
tools/gen_golden_infer.py), the colour table, BatchNorm folding, scripts/infer.py end to end, and the argument checks of the
three C-ABI entries (no GPU needed: nothing is launched on a bad argument)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import infer
from tests.infer_util import CONFIGS, ROOT, build_model, colour_mismatch, golden, randomize_batchnorm, smooth_image


# ---- host statements against the recorded reference outputs -------------------------------------------------------------------

def test_preprocess_equals_recorded_transform():
    g = golden()
    out = infer.preprocess_torch(g["pre_img"], 32, 64)
    assert out.dtype == torch.float32 and tuple(out.shape) == (1, 3, 32, 64)
    assert torch.equal(out, torch.from_numpy(g["pre_out"]))                       # the same torch calls: bit for bit
    both = infer.preprocess_torch(g["pre_img"], 32, 64, mirror=True)
    assert torch.equal(both[:1], out) and torch.equal(both[1:], out.flip(3))


def test_postprocess_paired_equals_recorded_blend():
    g = golden()
    disp, depth = infer.postprocess_torch(torch.from_numpy(g["pp_net"]), 37, 53, paired=True)
    err = float((disp - torch.from_numpy(g["pp_disp"])).abs().max())
    print("paired disparity vs reference: max abs %.3e" % err)
    assert err <= 1e-6           # the reference blends in float64; disparities in [0,1], a few float32 roundings
    a, b = infer.disp_to_depth_affine(0.1, 100.0)
    assert torch.allclose(depth, 1.0 / (a * disp + b), rtol=1e-6, atol=0)


def test_predict_equals_recorded_reference_predict():
    """The reference's predict() (320 x 1024 inside) with a channel-mean model, under its own depth scaling."""
    g = golden()

    class Mean(torch.nn.Module):
        def forward(self, inputs):
            return {("disp", 0, 0): inputs["color_aug", 0, 0].mean(1, keepdim=True)}

    p = infer.DepthPredictor(Mean(), 320, 1024, "cpu", affine=infer.REFERENCE_AFFINE, depth_scale=infer.REFERENCE_DEPTH_SCALE)
    pred = p.predict([g["pred_img"]])
    assert tuple(pred.disp.shape) == (1, 24, 40) and tuple(pred.disp_net.shape) == (1, 1, 320, 1024)
    np.testing.assert_allclose(pred.disp[0].numpy(), g["pred_disp"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(pred.depth[0].numpy(), g["pred_depth"], rtol=1e-5, atol=0)


# ---- colour map --------------------------------------------------------------------------------------------------------------

def test_committed_table_is_matplotlibs_magma():
    matplotlib = pytest.importorskip("matplotlib")
    want = matplotlib.colormaps["magma"](np.arange(256), bytes=True)[:, :3]
    assert np.array_equal(infer.magma_lut(), want)


def test_colorize_numpy_against_recorded_imsave():
    g = golden()
    lut = infer.magma_lut()
    differ = far = total = 0
    for i in range(2):
        field, want = g["col_field%d" % i], g["col_rgb%d" % i]
        mine = infer.colorize_numpy(field, field.min(), np.percentile(field, 95))
        assert mine.shape == want.shape and mine.dtype == np.uint8
        d, f = colour_mismatch(mine, want, lut)
        differ, far, total = differ + d, far + f, total + field.size
    print("colorize_numpy vs imsave: %d of %d pixels differ, %d by more than one index" % (differ, total, far))
    assert far == 0
    assert differ <= 1e-4 * total


def test_colorize_predictor_on_host_uses_minimum_and_percentile():
    g = golden()
    p = infer.DepthPredictor(torch.nn.Identity(), 32, 64, "cpu")
    field = g["col_field1"]
    pic = p.colorize(torch.from_numpy(field))
    assert tuple(pic.shape) == field.shape + (3,) and pic.dtype == torch.uint8
    assert np.array_equal(pic.numpy(), infer.colorize_numpy(field, field.min(), np.percentile(field, 95)))
    batch = p.colorize(torch.from_numpy(np.stack([field, 0.5 * field])))
    assert np.array_equal(batch[0].numpy(), pic.numpy()) and tuple(batch.shape) == (2,) + field.shape + (3,)


# ---- BatchNorm folding -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("config", CONFIGS)
def test_fold_batchnorm_equals_eval_forward_in_float64(config):
    from mono.model import networks
    model = randomize_batchnorm(build_model(config, 64, 96)).double().eval()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    n_bn = infer.count_batchnorms(model.DepthEncoder)
    assert n_bn >= 20
    folded = infer.fold_batchnorm(model)
    assert infer.count_batchnorms(folded.DepthEncoder) == 0 and infer.count_batchnorms(folded.DepthDecoder) == 0
    assert sum(isinstance(m, torch.nn.Identity) for m in folded.DepthEncoder.modules()) == n_bn
    assert not any(isinstance(m, networks.BatchNorm) for m in folded.modules())       # every pair of the other sub-networks too
    x = infer.network_inputs(torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(5), dtype=torch.float64))
    with torch.no_grad():
        want, got = model(x), folded(x)
    for s in range(4):
        err = float((want[("disp", 0, s)] - got[("disp", 0, s)]).abs().max())
        print("%s scale %d: folded vs eval max abs %.3e" % (config, s, err))
        assert err <= 1e-9
    assert float((want[("disp", 0, 0)].max() - want[("disp", 0, 0)].min())) > 1e-4      # not a constant map
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not model.training


def test_fold_leaves_an_unpaired_batchnorm_alone():
    from mono.model import networks
    lone = torch.nn.Sequential(networks.BatchNorm(4), torch.nn.ReLU(), torch.nn.Conv2d(4, 4, 1))
    assert infer.count_batchnorms(infer.fold_batchnorm(lone)) == 1


def test_predictor_keeps_the_callers_model():
    model = randomize_batchnorm(build_model("cfg_kitti_fm", 64, 96))
    model.train()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    p = infer.DepthPredictor(model, 64, 96, "cpu")
    pred = p.predict([smooth_image(3, 37, 53)])
    assert model.training and p.model is not model and not p.model.training
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    assert tuple(pred.disp.shape) == (1, 37, 53) and tuple(pred.depth.shape) == (1, 37, 53)
    assert not pred.disp.requires_grad
    with pytest.raises(ValueError):
        infer.DepthPredictor(model, 64, 96, "cpu", precision="bf16")


# ---- the network the evaluators run ------------------------------------------------------------------------------------------

def test_eval_network_fp32_runs_the_callers_model_and_restores_it():
    model = build_model("cfg_kitti_fm", 32, 64).train()
    net, restore = infer.eval_network(model, "cpu", "fp32")
    assert net is model
    with restore:
        assert not any(m.training for m in model.modules())
    assert model.training and all(m.training for m in model.modules())
    net, restore = infer.eval_network(model, torch.device("cpu"), "fp32")
    with pytest.raises(RuntimeError, match="inside"):
        with restore:
            assert not model.training
            raise RuntimeError("inside")
    assert net is model and all(m.training for m in model.modules())
    net, restore = infer.eval_network(model.eval(), "cpu", "fp32")
    with restore:
        pass
    assert not any(m.training for m in model.modules())          # the previous flag, not "training", comes back


def test_eval_network_bf16_runs_a_folded_copy():
    model = randomize_batchnorm(build_model("cfg_kitti_fm", 32, 64)).train()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    n_bn = infer.count_batchnorms(model.DepthEncoder)
    net, restore = infer.eval_network(model, "cpu", "bf16")
    with restore:
        assert net is not model and not any(m.training for m in net.modules())
        assert n_bn > 0 and infer.count_batchnorms(net.DepthEncoder) == 0
        assert sum(isinstance(m, torch.nn.Identity) for m in net.DepthEncoder.modules()) == n_bn
        assert all(m.training for m in model.modules())
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) and after[k].dtype == before[k].dtype for k in before)
    assert all(m.training for m in model.modules()) and infer.count_batchnorms(model.DepthEncoder) == n_bn
    assert next(model.parameters()).dtype == torch.float32


# ---- script ------------------------------------------------------------------------------------------------------------------

def test_infer_script_on_cpu(tmp_path):
    from PIL import Image
    model = randomize_batchnorm(build_model("cfg_kitti_fm", 192, 640, seed=7))
    ckpt = tmp_path / "random.pth"
    torch.save({"state_dict": model.state_dict()}, str(ckpt))
    rgb = smooth_image(11, 75, 131)
    Image.fromarray(rgb).save(str(tmp_path / "frame.png"))
    out = tmp_path / "out"
    cfg = os.path.join(ROOT, "config", "cfg_kitti_fm.py")
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "infer.py"), "--config", cfg, "--checkpoint", str(ckpt),
                    "--device", "cpu", "--image", str(tmp_path / "frame.png"), "--out", str(out), "--save_depth"],
                   check=True, env=env, timeout=600)
    pic = np.asarray(Image.open(str(out / "frame_disp.png")))
    depth = np.load(str(out / "frame_depth.npy"))
    assert pic.shape == (75, 131, 3) and depth.shape == (75, 131) and depth.dtype == np.float32
    p = infer.DepthPredictor.from_config(cfg, str(ckpt), device="cpu")
    assert (p.height, p.width) == (192, 640)
    pred = p.predict([rgb])
    assert np.array_equal(depth, pred.depth[0].numpy())
    assert np.array_equal(pic, p.colorize(pred.disp[0]).numpy())
    assert float(depth.min()) >= 0.1 - 1e-6 and float(depth.max()) <= 100.0 + 1e-3


def test_infer_script_split_mode_on_cpu(tmp_path):
    """--split over the configuration's validation dataset (synthetic frames here): img_%04d.jpg and disp_%04d.jpg at the network size."""
    from PIL import Image
    ckpt = tmp_path / "random.pth"
    torch.save({"state_dict": build_model("cfg_kitti_fm", 192, 640, seed=7).state_dict()}, str(ckpt))
    out = tmp_path / "split"
    env = dict(os.environ, PYTHONPATH=ROOT, TD_ALLOW_SYNTHETIC="1", KITTI_RAW=str(tmp_path / "no_kitti_here"))
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "infer.py"), "--config", os.path.join(ROOT, "config", "cfg_kitti_fm.py"),
                    "--checkpoint", str(ckpt), "--device", "cpu", "--split", "--post_process", "--out", str(out)],
                   check=True, env=env, timeout=900)
    names = sorted(os.listdir(str(out)))
    n = len(names) // 2
    assert n >= 1 and names == ["disp_%04d.jpg" % i for i in range(n)] + ["img_%04d.jpg" % i for i in range(n)]
    for name in (names[0], names[-1]):
        assert Image.open(str(out / name)).size == (640, 192)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------

def test_new_entries_reject_bad_arguments():
    from tripled_amd import native
    lib = native.load()
    assert lib.td_abi_version() == 3
    one = 0x1000      # a non-null address: the size checks come before any launch
    assert lib.td_infer_preprocess(None, 1, 8, 8, 4, 4, 0, None, None) == -1
    assert lib.td_infer_preprocess(one, 0, 8, 8, 4, 4, 0, one, None) == -1
    assert lib.td_infer_preprocess(one, 1, 8, 8, 0, 4, 0, one, None) == -1
    assert lib.td_infer_preprocess(one, 1, 8, 8, 4, 4, 2, one, None) == -1
    assert lib.td_disp_postprocess(None, 0, 1, 4, 4, 0, 8, 8, 1.0, 1.0, 1.0, None, None, None) == -1
    assert lib.td_disp_postprocess(one, 0, 1, 4, 4, 0, 8, 8, 1.0, 1.0, 1.0, None, None, None) == -1
    assert lib.td_disp_postprocess(one, 0, 1, 4, 4, 0, 8, -1, 1.0, 1.0, 1.0, one, None, None) == -1
    assert lib.td_disp_postprocess(one, 7, 1, 4, 4, 0, 8, 8, 1.0, 1.0, 1.0, one, None, None) == -2      # unknown dtype
    assert lib.td_disp_postprocess(one, 0, 1, 4, 1, 1, 8, 8, 1.0, 1.0, 1.0, one, None, None) == -2      # the ramp needs w >= 2
    assert lib.td_colorize(None, 1, 16, None, None, None, None, None) == -1
    assert lib.td_colorize(one, 1, 0, one, one, one, one, None) == -1
    assert lib.td_colorize(one, 1, 16, one, None, one, one, None) == -1
    with pytest.raises(native.NativeLibraryError):                # the kernels take device tensors only: no quiet host path
        infer.preprocess_hip(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 4, 4)
