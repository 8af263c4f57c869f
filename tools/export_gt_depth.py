#!/usr/bin/env python3
"""Writes the ground-truth archive of a split from the raw KITTI tree's velodyne scans (the reference has no such program; the usual
gt_depths.npz is monodepth2's export of the same function, an object array that needs pickle).

  python tools/export_gt_depth.py --config config/cfg_kitti_tripleD.py [--split_file F] --out gt_depths.npz [--device cpu]

The frames are the configuration's validation split (cfg.data.split, cfg.data.split_dir) or the lines of --split_file, "<folder>
<frame_index> <l|r>" each, in order.  The archive is pickle-free, what MonoDataset loads with allow_pickle=False:
  data   float32 [n,Hmax,Wmax]   the maps at native size, zero-padded at the bottom and right to the largest
  sizes  int32 [n,2]             (H, W) of every map; the dataset serves data[i, :H, :W]
On a HIP device the maps are made in batches by csrc/td_velo.hip (tripled_amd.velodyne.VelodyneGroundTruth), on 'cpu' by the numpy
statement; the two are equal bit for bit.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tripled_amd  # noqa: F401,E402
from tripled_amd import velodyne  # noqa: E402


def export(data_path, filenames, out, device="cpu", batch_size=12):
    """filenames: split lines.  Returns (data, sizes) as written to ``out``."""
    items = []
    for line in filenames:
        folder, frame_index, side = line.split()
        items.append((folder, int(frame_index), side))
    if not items:
        raise ValueError("no frames to export")
    make = velodyne.VelodyneGroundTruth(data_path, device)
    maps = []
    for at in range(0, len(items), int(batch_size)):
        got = make(items[at:at + int(batch_size)])
        if isinstance(got, list):
            maps.extend(got)
        else:
            gt, sizes, _ = got
            gt, sizes = gt.cpu().numpy(), sizes.cpu().numpy()
            maps.extend(gt[i, :h, :w] for i, (h, w) in enumerate(sizes))
    sizes = np.array([m.shape for m in maps], dtype=np.int32)
    data = np.zeros((len(maps), int(sizes[:, 0].max()), int(sizes[:, 1].max())), np.float32)
    for i, m in enumerate(maps):
        data[i, :m.shape[0], :m.shape[1]] = m
    np.savez_compressed(out, data=data, sizes=sizes)
    return data, sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--split_file", default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--batch_size", type=int, default=12)
    args = ap.parse_args()
    from mmcv import Config
    from mono.datasets.kitti_dataset import read_split
    cfg = Config.fromfile(args.config)
    if args.split_file:
        with open(args.split_file) as f:
            filenames = [line for line in f.read().splitlines() if line.strip()]
    else:
        filenames = read_split(cfg.data["split"], "val", cfg.data.get("split_dir", None))
    data, sizes = export(cfg.data["in_path"], filenames, args.out, args.device, args.batch_size)
    print("%s: %d maps, padded to %d x %d, %d bytes" % (args.out, len(data), data.shape[1], data.shape[2], os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
