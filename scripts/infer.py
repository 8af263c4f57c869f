#!/usr/bin/env python3
"""Depth prediction from a trained checkpoint: the disparity picture (magma, vmax at the 95th percentile) and, on request, the
depth map.

  python scripts/infer.py --config config/cfg_kitti_tripleD.py --checkpoint work/epoch_20.pth --image assets/test.png --out out
  python scripts/infer.py --config config/cfg_kitti_tripleD.py --checkpoint work/epoch_20.pth --split --out out

The reference has two programs for this, scripts/infer.py (one image -> test_disp.png) and scripts/infer_singleimage.py (the
validation split -> img_%04d.jpg / disp_%04d.jpg).  Both are the same three steps -- image to network input, forward, disparity
to picture -- around a different source of images, and both repeat the model loading; here they are the two modes of one
program over tripled_amd.infer.DepthPredictor, so the steps exist once:
  --image FILE|DIR   writes NAME_disp.png per image (NAME_depth.npy with --save_depth).  The disparity is resized back to the
                     image's own size, as the reference's predict() does.  --reference_formula applies the reference infer.py's
                     depth scaling, 36 / (disp / 1e-3 + 1 / 80), instead of disp_to_depth(., min_depth, max_depth) of the config.
  --split            writes img_%04d.jpg and disp_%04d.jpg for every sample of the configuration's validation dataset.
Deviation from the reference's infer.py: the network size is the configuration's (cfg.data height / width), not a hard-coded
320 x 1024.  --post_process adds the flip post-processing of the reference's scripts/eval_depth_pp.py.  Images are read and
written with PIL.
"""
import argparse
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tripled_amd  # noqa: F401,E402
from tripled_amd import infer  # noqa: E402

IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".ppm")


def image_files(path):
    if os.path.isdir(path):
        return sorted(os.path.join(path, f) for f in os.listdir(path) if f.lower().endswith(IMAGE_EXTENSIONS))
    return [path]


def run_images(predictor, path, out_dir, save_depth=False):
    written = []
    for file in image_files(path):
        rgb = np.asarray(Image.open(file).convert("RGB"))
        pred = predictor.predict([rgb])
        name = os.path.splitext(os.path.basename(file))[0]
        target = os.path.join(out_dir, name + "_disp.png")
        Image.fromarray(predictor.colorize(pred.disp[0]).cpu().numpy()).save(target)
        written.append(target)
        if save_depth:
            np.save(os.path.join(out_dir, name + "_depth.npy"), pred.depth[0].cpu().numpy())
    return written


def run_split(predictor, dataset, out_dir):
    """reference scripts/infer_singleimage.py:56-71: the network-size frame and the picture of its scaled disparity."""
    for idx in range(len(dataset)):
        sample = dataset[idx]
        if ("color_u8", 0) in sample:
            frame = torch.as_tensor(sample[("color_u8", 0)])
        else:
            frame = (torch.as_tensor(sample[("color", 0, 0)]).float() * 255.0).round().clamp_(0, 255).to(torch.uint8)
        rgb = frame.permute(1, 2, 0).contiguous().numpy()
        pred = predictor.predict([rgb])
        Image.fromarray(rgb).save(os.path.join(out_dir, "img_{:0>4d}.jpg".format(idx)))
        scaled = pred.disp[0] * predictor.a + predictor.b                  # disp_to_depth's scaled disparity
        Image.fromarray(predictor.colorize(scaled).cpu().numpy()).save(os.path.join(out_dir, "disp_{:0>4d}.jpg".format(idx)))
    return len(dataset)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16"))
    ap.add_argument("--post_process", action="store_true")
    ap.add_argument("--out", required=True, metavar="DIR")
    what = ap.add_mutually_exclusive_group(required=True)
    what.add_argument("--image", metavar="FILE|DIR")
    what.add_argument("--split", action="store_true")
    ap.add_argument("--save_depth", action="store_true")
    ap.add_argument("--reference_formula", action="store_true")
    args = ap.parse_args(argv)
    kwargs = dict(precision=args.precision, post_process=args.post_process)
    if args.reference_formula:
        kwargs.update(affine=infer.REFERENCE_AFFINE, depth_scale=infer.REFERENCE_DEPTH_SCALE)
    predictor = infer.DepthPredictor.from_config(args.config, args.checkpoint, device=args.device, **kwargs)
    os.makedirs(args.out, exist_ok=True)
    if args.split:
        from mmcv import Config
        from mono.datasets.get_dataset import get_dataset
        n = run_split(predictor, get_dataset(Config.fromfile(args.config).data, training=False), args.out)
        print("-> %d frames written to %s" % (n, args.out))
    else:
        for target in run_images(predictor, args.image, args.out, args.save_depth):
            print("->", target)


if __name__ == "__main__":
    main()
