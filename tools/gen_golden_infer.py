#!/usr/bin/env python3
"""Records tests/golden/infer.npz: small inputs and what the REFERENCE's inference programs make of them, so that the tests
of tripled_amd.infer (CPU and GPU) have the reference's numbers where its checkout is not present.

  python tools/gen_golden_infer.py --reference /path/to/reference [--out tests/golden/infer.npz]

The reference's scripts/infer.py and scripts/eval_depth_pp.py are loaded stand-alone (``load_reference``): their imports of
cv2, mmcv and the reference's own ``mono`` package are satisfied by stub modules, and Tensor.cuda() is a no-op, so their
functions run on the host.  Recorded (data only):
  pre_img / pre_out          uint8 image 37 x 53 -> transform(img, 32, 64)
  pp_net / pp_disp           network disparities [2 B,1,32,64] (second half: predictions of the mirrored images) ->
                             batch_post_process_disparity(l, un-mirrored r), as float32, resized to 37 x 53 like predict() does
  pred_img / pred_depth / pred_disp   uint8 image 24 x 40 -> predict(img, model) with model = channel mean (320 x 1024 inside)
  col_field<i> / col_rgb<i>  smooth fields -> the RGB bytes of plt.imsave(., cmap='magma', vmax=np.percentile(., 95))
"""
import argparse
import importlib.util
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = {
    "cv2": dict(setNumThreads=lambda n: None),
    "mmcv": dict(Config=None),
    "mono.model.registry": dict(MONO=None),
    "mono.model.mono_baseline.layers": dict(disp_to_depth=None),
    "mono.datasets.utils": dict(readlines=None, compute_errors=None),
    "mono.datasets.kitti_dataset": dict(KITTIRAWDataset=None),
}


def load_reference(reference_root, patcher):
    """(scripts/infer.py, scripts/eval_depth_pp.py) of the reference as modules.  ``patcher`` is a pytest MonkeyPatch: the stub
    modules and the no-op Tensor.cuda last until it is undone."""
    for name, attrs in STUBS.items():
        stub = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(stub, k, v)
        patcher.setitem(sys.modules, name, stub)
    patcher.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    patcher.setattr(sys, "dont_write_bytecode", True)
    mods = []
    for file in ("infer.py", "eval_depth_pp.py"):
        spec = importlib.util.spec_from_file_location("_reference_" + file[:-3], os.path.join(reference_root, "scripts", file))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return tuple(mods)


def smooth_field(seed, h, w):
    """A disparity-like float32 field in (0, 1): a few low-frequency waves plus a ramp."""
    g = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    f = 0.3 + 0.4 * y
    for _ in range(4):
        fy, fx, ph = g.uniform(0.5, 3.0), g.uniform(0.5, 3.0), g.uniform(0, 6.28)
        f = f + 0.07 * np.sin(6.28 * (fy * y + fx * x) + ph)
    return np.clip(f, 0.01, 0.99).astype(np.float32)


def smooth_image(seed, h, w):
    return np.stack([np.round(255 * smooth_field(seed + c, h, w)) for c in range(3)], -1).astype(np.uint8)


def channel_mean_model(inputs):
    return {("disp", 0, 0): inputs["color_aug", 0, 0].mean(1, keepdim=True)}


def imsave_rgb(field):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from PIL import Image
    buf = io.BytesIO()
    plt.imsave(buf, field, cmap="magma", vmax=np.percentile(field, 95), format="png")
    buf.seek(0)
    return np.asarray(Image.open(buf).convert("RGB"))


def record(ref_infer, ref_pp):
    out = {}
    out["pre_img"] = smooth_image(1, 37, 53)
    out["pre_out"] = ref_infer.transform(out["pre_img"], 32, 64).numpy()
    B, h, w = 2, 32, 64
    l = np.stack([smooth_field(10 + i, h, w) for i in range(B)])
    r_net = np.stack([smooth_field(20 + i, h, w) for i in range(B)])      # what the network returns for the mirrored images
    out["pp_net"] = np.concatenate([l, r_net])[:, None]
    blended = ref_pp.batch_post_process_disparity(l, r_net[:, :, ::-1])
    out["pp_disp"] = torch.nn.functional.interpolate(torch.from_numpy(blended.astype(np.float32))[:, None], (37, 53), mode="bilinear",
                                                     align_corners=False)[:, 0].numpy()
    out["pred_img"] = smooth_image(30, 24, 40)
    depth, disp = ref_infer.predict(out["pred_img"], channel_mean_model)
    out["pred_depth"], out["pred_disp"] = depth.astype(np.float32), disp.astype(np.float32)
    for i, (fh, fw) in enumerate([(48, 80), (45, 71)]):
        out["col_field%d" % i] = smooth_field(40 + i, fh, fw)
        out["col_rgb%d" % i] = imsave_rgb(out["col_field%d" % i])
    return out


def main():
    import pytest
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "infer.npz"))
    args = ap.parse_args()
    patcher = pytest.MonkeyPatch()
    try:
        data = record(*load_reference(args.reference, patcher))
    finally:
        patcher.undo()
    np.savez_compressed(args.out, **data)
    print("%s: %d arrays, %d bytes" % (args.out, len(data), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
