#!/usr/bin/env python3
"""Offline KITTI depth evaluation (reference: scripts/eval_depth.py:22-109): load a checkpoint, predict the
disparity of every validation frame, resize to the ground-truth size, median-scale (x36 for stereo), clamp to
[1e-3, 80] inside the Garg crop and print the seven standard metrics.

  python scripts/eval_depth.py --config config/cfg_kitti_tripleD.py --checkpoint work/epoch_20.pth \
         --gt_depths /data/kitti_raw/gt_depths.npz [--batch_size 12 [--precision bf16] [--post_process]]
  python scripts/eval_depth.py --config config/cfg_kitti_tripleD.py --checkpoint work/epoch_20.pth --gt velodyne [--batch_size 12]

--gt velodyne needs no archive: the ground truth is made from the raw tree's velodyne scans (tripled_amd.velodyne) -- per batch on
the device by csrc/td_velo.hip with --batch_size N, per frame by KITTIRAWDataset.get_depth in the loop below.

--batch_size N scores N frames per launch chain on the device (tripled_amd.evaluate.DepthEvaluator, csrc/td_eval.hip); the
default, 0, is the loop below.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tripled_amd  # noqa: F401,E402
from mmcv import Config  # noqa: E402
from mono.core.evaluation import disp_to_depth, evaluate_disparity  # noqa: E402
from mono.core.evaluation.eval_hooks import METRICS  # noqa: E402
from mono.datasets.device_expand import GROUND_TRUTH_KEYS  # noqa: E402
from mono.datasets.get_dataset import get_dataset  # noqa: E402
from mono.model import MONO  # noqa: E402


def evaluate(model, dataset, stereo_scale=False, device="cuda"):
    """Returns (mean metrics dict, scale ratios) over a validation dataset whose samples carry 'gt_depth', or (cfg.data.gt_source =
    'velodyne') a raw scan: the ground truth is then dataset.get_depth of the sample's line."""
    model.eval().to(device)
    results = []
    with torch.no_grad():
        for idx in range(len(dataset)):
            sample = dataset[idx]
            batch = {k: torch.as_tensor(v).float().unsqueeze(0).to(device) for k, v in sample.items() if k not in GROUND_TRUTH_KEYS}
            scaled, _ = disp_to_depth(model(batch)[("disp", 0, 0)].float(), 0.1, 100)
            if "gt_depth" in sample:
                gt = np.asarray(sample["gt_depth"], dtype=np.float32)
            else:
                folder, frame_index, side = dataset.filenames[idx].split()
                gt = dataset.get_depth(folder, int(frame_index), side, False)
            results.append(evaluate_disparity(scaled.cpu()[0, 0].numpy(), gt, stereo_scale))
    mean = {k: float(np.mean([r[k] for r in results])) for k in METRICS}
    return mean, np.array([r["scale"] for r in results])


def evaluate_batched(model, dataset, stereo_scale=False, device="cuda", batch_size=12, precision="fp32", post_process=False):
    """evaluate() in batches through tripled_amd.evaluate.DepthEvaluator: scored on the device by td_eval_depth."""
    from tripled_amd.evaluate import DepthEvaluator
    return DepthEvaluator(model.eval().to(device), device, batch_size=batch_size, precision=precision, post_process=post_process,
                          stereo_scale=stereo_scale).evaluate(dataset)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--gt_depths", default=None)
    ap.add_argument("--gt", choices=("archive", "velodyne"), default=None,
                    help="where the ground truth comes from (default: cfg.data.gt_source, else the archive); velodyne: the raw scans")
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--batch_size", type=int, default=0,
                    help="0: one frame at a time, scored on the host; N > 0: batches of N scored on the device (DepthEvaluator)")
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32", help="with --batch_size: the forward's precision")
    ap.add_argument("--post_process", action="store_true", help="with --batch_size: flip post-processing (eval_depth_pp.py)")
    args = ap.parse_args()
    if args.batch_size <= 0 and (args.precision != "fp32" or args.post_process):
        ap.error("--precision bf16 and --post_process belong to the batched path: give --batch_size N")
    cfg = Config.fromfile(args.config)
    if args.gt_depths:
        cfg.data["gt_depth_path"] = args.gt_depths
    if args.gt:
        cfg.data["gt_source"] = args.gt
    cfg.model["imgs_per_gpu"] = 1
    model = MONO.module_dict[cfg.model["name"]](cfg.model)
    ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=True)      # executes nothing from the file
    model.load_state_dict(ckpt["state_dict"], strict=True)
    dataset, stereo = get_dataset(cfg.data, training=False), bool(cfg.data["stereo_scale"])
    if args.batch_size > 0:
        mean, ratios = evaluate_batched(model, dataset, stereo, args.device, args.batch_size, args.precision, args.post_process)
    else:
        mean, ratios = evaluate(model, dataset, stereo, args.device)
    med = np.median(ratios)
    print("Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(med, np.std(ratios / med)))
    print("\n  " + ("{:>8} | " * 7).format(*METRICS))
    print(("&{: 8.3f}  " * 7).format(*[mean[k] for k in METRICS]) + "\\\\")


if __name__ == "__main__":
    main()
