"""Shared pieces of the inference tests (test_infer_cpu.py, test_infer_vs_reference.py, test_hip_infer.py)."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ("cfg_kitti_fm", "cfg_kitti_tripleD", "cfg_kitti_fm_joint_inpaint_disentangle_distill_full_colorize")


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "infer.npz"))


def build_model(config, height, width, seed=0, **overrides):
    """The model class of config/<config>.py at a small network size, seeded random initialisation."""
    import tripled_amd  # noqa: F401
    from mmcv import Config
    from mono.model import MONO
    cfg = Config.fromfile(os.path.join(ROOT, "config", config + ".py"))
    cfg.model.update(height=height, width=width, imgs_per_gpu=1, **overrides)
    torch.manual_seed(seed)
    return MONO.module_dict[cfg.model["name"]](cfg.model)


def randomize_batchnorm(model, seed=1):
    """Non-trivial running statistics and affine parameters for every BatchNorm (a fresh model has mean 0, var 1, weight 1,
    bias 0, with which folding would be the identity)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                n = m.num_features
                m.running_mean.copy_(0.2 * torch.randn(n, generator=g))
                m.running_var.copy_(0.5 + torch.rand(n, generator=g))
                m.weight.copy_(0.7 + 0.6 * torch.rand(n, generator=g))
                m.bias.copy_(0.1 * torch.randn(n, generator=g))
    return model


def smooth_image(seed, h, w, batch=None):
    """uint8 H x W x 3 (or B x H x W x 3): low-frequency waves plus a little noise, full byte range."""
    g = np.random.default_rng(seed)
    n = batch or 1
    y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    out = np.empty((n, h, w, 3), np.float64)
    for i in range(n):
        for c in range(3):
            fy, fx, ph = g.uniform(0.5, 4.0), g.uniform(0.5, 4.0), g.uniform(0, 6.28)
            out[i, :, :, c] = 127.5 + 110 * np.sin(6.28 * (fy * y + fx * x) + ph) + g.uniform(-17, 17, (h, w))
    out = np.clip(np.round(out), 0, 255).astype(np.uint8)
    return out if batch else out[0]


def smooth_disp(seed, n, h, w):
    """float32 [n,1,h,w] in (0, 1)."""
    g = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    out = np.empty((n, 1, h, w), np.float64)
    for i in range(n):
        f = 0.3 + 0.4 * y
        for _ in range(4):
            fy, fx, ph = g.uniform(0.5, 3.0), g.uniform(0.5, 3.0), g.uniform(0, 6.28)
            f = f + 0.07 * np.sin(6.28 * (fy * y + fx * x) + ph)
        out[i, 0] = f
    return torch.from_numpy(np.clip(out, 0.01, 0.99).astype(np.float32))


def colour_mismatch(mine, ref, lut):
    """(pixels that differ, pixels that differ by MORE than one table index) between two uint8 [..., 3] pictures drawn from
    ``lut``.  A table colour may occur at several indices: any index of ``mine``'s colour next to any of ``ref``'s counts."""
    mine, ref = mine.reshape(-1, 3), ref.reshape(-1, 3)
    differ = np.nonzero((mine != ref).any(1))[0]
    far = 0
    for p in differ:
        a = np.nonzero((lut == mine[p]).all(1))[0]
        b = np.nonzero((lut == ref[p]).all(1))[0]
        if not (len(a) and len(b) and np.abs(a[:, None] - b[None, :]).min() <= 1):
            far += 1
    return len(differ), far
