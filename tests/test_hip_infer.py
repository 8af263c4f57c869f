"""The three inference kernels of csrc/td_infer.hip (through ctypes: tripled_amd.infer.*_hip) against the host statements of
tripled_amd.infer on the same device and against the reference's recorded outputs (tests/golden/infer.npz), then the
DepthPredictor on the device: its composition and its BatchNorm-folded bf16 forward.

Bounds.  preprocess: atol 1e-5 on [0,1] values (a handful of float32 roundings of values <= 255, then / 255: ~1e-7 each, 400 x
below the 1/255 quantum).  postprocess: disp atol 1e-6 (disparities in [0,1], a few float32 roundings), depth rtol 1e-5.
colorize: at most one table index per pixel on at most 1e-4 of the pixels (bit-equality expected: every step is a correctly
rounded float32 operation)."""
import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import infer
from tests.infer_util import CONFIGS, build_model, colour_mismatch, golden, randomize_batchnorm, smooth_disp, smooth_image

pytestmark = pytest.mark.gpu

# input size -> network size
SHAPES = [(375, 1242, 192, 640), (375, 1242, 320, 1024), (37, 53, 32, 64), (64, 100, 96, 320)]
BATCHES = [1, 2, 12]
AFFINES = [infer.REFERENCE_AFFINE + (infer.REFERENCE_DEPTH_SCALE,), infer.disp_to_depth_affine(0.1, 100.0) + (1.0,)]


def _dev():
    return torch.device("cuda", 0)


# ---- 1. preprocess -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_preprocess_kernel(shape, B, mirror):
    H0, W0, h, w = shape
    img = torch.from_numpy(smooth_image(B + h, H0, W0, batch=B)).to(_dev())
    got = infer.preprocess_hip(img, h, w, mirror)
    want = infer.preprocess_torch(img, h, w, mirror)
    assert got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous()
    err = float((got - want).abs().max())
    print("preprocess %s B %d mirror %d: max abs %.3e" % (shape, B, mirror, err))
    assert err <= 1e-5
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0 and float(got.max() - got.min()) > 0.5
    if mirror:
        assert torch.equal(got[B:], got[:B].flip(3))


def test_preprocess_kernel_scalar_store_path():
    """A network width that is not a multiple of 4 takes the one-column-per-thread variant."""
    img = torch.from_numpy(smooth_image(2, 37, 53, batch=2)).to(_dev())
    got, want = infer.preprocess_hip(img, 30, 61, True), infer.preprocess_torch(img, 30, 61, True)
    assert float((got - want).abs().max()) <= 1e-5 and torch.equal(got[2:], got[:2].flip(3))


def test_preprocess_kernel_against_recorded_transform():
    g = golden()
    got = infer.preprocess_hip(torch.from_numpy(g["pre_img"])[None].to(_dev()), 32, 64)
    err = float((got.cpu() - torch.from_numpy(g["pre_out"])).abs().max())
    print("preprocess vs reference transform: max abs %.3e" % err)
    assert err <= 1e-5


# ---- 2. postprocess ------------------------------------------------------------------------------------------------------------

def _check_post(got, want, what):
    (gd, gz), (wd, wz) = got, want
    assert gd.shape == wd.shape and gz.shape == wz.shape and gd.dtype == torch.float32
    err_d = float((gd - wd).abs().max())
    err_z = float(((gz - wz).abs() / wz.abs()).max())
    print("postprocess %s: disp max abs %.3e, depth max rel %.3e" % (what, err_d, err_z))
    assert err_d <= 1e-6
    assert err_z <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_postprocess_kernel(shape, B, paired, dtype):
    H0, W0, h, w = shape
    net = smooth_disp(B + h + paired, B * (2 if paired else 1), h, w).to(_dev()).to(dtype)
    for a, b, scale in AFFINES:
        got = infer.postprocess_hip(net, H0, W0, paired, a, b, scale)
        want = infer.postprocess_torch(net, H0, W0, paired, a, b, scale)
        _check_post(got, want, "%s B %d paired %d %s scale %g" % (shape, B, paired, dtype, scale))
    only_disp, none = infer.postprocess_hip(net, H0, W0, paired, want_depth=False)
    assert none is None and torch.equal(only_disp, got[0])


def test_postprocess_kernel_against_recorded_reference():
    g = golden()
    disp, _ = infer.postprocess_hip(torch.from_numpy(g["pp_net"]).to(_dev()), 37, 53, paired=True)
    err = float((disp.cpu() - torch.from_numpy(g["pp_disp"])).abs().max())
    print("paired postprocess vs reference: max abs %.3e" % err)
    assert err <= 1e-6
    # the reference's predict(): 320 x 1024 inside, channel-mean model, depth = 36 / (disp / 1e-3 + 1 / 80)
    x = infer.preprocess_hip(torch.from_numpy(g["pred_img"])[None].to(_dev()), 320, 1024)
    a, b = infer.REFERENCE_AFFINE
    d, z = infer.postprocess_hip(x.mean(1, keepdim=True), 24, 40, False, a, b, infer.REFERENCE_DEPTH_SCALE)
    err_d = float((d[0].cpu() - torch.from_numpy(g["pred_disp"])).abs().max())
    err_z = float(((z[0].cpu() - torch.from_numpy(g["pred_depth"])).abs() / torch.from_numpy(g["pred_depth"])).max())
    print("predict vs reference: disp max abs %.3e, depth max rel %.3e" % (err_d, err_z))
    assert err_d <= 1e-6 and err_z <= 1e-5


# ---- 3. colorize ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("size", [(375, 1242), (37, 53), (64, 100)])
def test_colorize_kernel(size, B):
    field = smooth_disp(B + size[0], B, *size)[:, 0]
    flat = field.reshape(B, -1)
    vmin = flat.amin(1)
    vmax = torch.stack([torch.quantile(r, 0.95) for r in flat])
    got = infer.colorize_hip(field.to(_dev()), vmin.to(_dev()), vmax.to(_dev())).cpu().numpy()
    want = infer.colorize_numpy(field.numpy(), vmin.numpy(), vmax.numpy())
    assert got.shape == want.shape == (B,) + size + (3,) and got.dtype == np.uint8
    differ, far = colour_mismatch(got, want, infer.magma_lut())
    print("colorize %s B %d: %d of %d pixels differ, %d by more than one index" % (size, B, differ, flat.numel(), far))
    assert far == 0 and differ <= 1e-4 * flat.numel()
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 100           # the picture uses the table


def test_colorize_kernel_against_recorded_imsave():
    g = golden()
    p = infer.DepthPredictor(torch.nn.Identity(), 32, 64, _dev())
    differ = far = total = 0
    for i in range(2):
        field = g["col_field%d" % i]
        pic = p.colorize(torch.from_numpy(field).to(_dev())).cpu().numpy()          # torch.quantile + td_colorize
        d, f = colour_mismatch(pic, g["col_rgb%d" % i], infer.magma_lut())
        differ, far, total = differ + d, far + f, total + field.size
    print("colorize vs imsave: %d of %d pixels differ, %d by more than one index" % (differ, total, far))
    assert far == 0 and differ <= 1e-4 * total


# ---- 4. composition ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("post_process", [False, True])
def test_predictor_composition(post_process):
    model = build_model("cfg_kitti_tripleD", 192, 640, seed=3).to(_dev()).eval()
    p = infer.DepthPredictor(model, 192, 640, _dev(), post_process=post_process)
    img = smooth_image(5, 375, 1242, batch=2)
    x = p.preprocess(img)
    assert tuple(x.shape) == (4 if post_process else 2, 3, 192, 640)
    with torch.no_grad():
        net = model(infer.network_inputs(x))[("disp", 0, 0)]
    want = infer.postprocess_torch(net, 375, 1242, post_process, p.a, p.b, p.depth_scale)
    pred = p.predict(img)
    assert tuple(pred.disp_net.shape) == tuple(net.shape) and pred.disp_net.dtype == torch.float32
    _check_post((pred.disp, pred.depth), want, "predictor post_process %d" % post_process)
    assert not model.training and float(pred.disp.std()) > 0


# ---- 5. bf16 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("config", CONFIGS)
def test_folded_bf16_forward_is_as_close_to_fp32_as_autocast(config):
    """Yardstick: the UNFOLDED model under bf16 autocast (existing code).  The folded bf16 path may be at most 1.5 x as far from
    the fp32 eval disparity, in the mean and in the maximum: folding rounds w * s to bf16 once instead of rounding w and applying s
    in fp32 -- the same order of error, not the same value."""
    model = randomize_batchnorm(build_model(config, 96, 320)).to(_dev()).eval()
    p = infer.DepthPredictor(model, 96, 320, _dev(), precision="bf16")
    assert infer.count_batchnorms(p.model.DepthEncoder) == 0
    x = p.preprocess(smooth_image(9, 120, 400, batch=2))
    xcl = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        d32 = model(infer.network_inputs(x))[("disp", 0, 0)].float()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            dA = model(infer.network_inputs(xcl))[("disp", 0, 0)].float()
    dF = p.forward(x).float()
    assert dF.shape == d32.shape
    mean_a, max_a = float((dA - d32).abs().mean()), float((dA - d32).abs().max())
    mean_f, max_f = float((dF - d32).abs().mean()), float((dF - d32).abs().max())
    print("%s: |autocast - fp32| mean %.3e max %.3e; |folded bf16 - fp32| mean %.3e max %.3e" % (config, mean_a, max_a, mean_f, max_f))
    assert mean_a > 0 and max_a > 0, "the yardstick distance is zero: autocast did not run in bf16"
    assert mean_f <= 1.5 * mean_a
    assert max_f <= 1.5 * max_a
    pred = p.predict(smooth_image(9, 120, 400, batch=2))
    assert pred.disp_net.dtype == torch.bfloat16 and tuple(pred.disp.shape) == (2, 120, 400) and pred.disp.dtype == torch.float32
