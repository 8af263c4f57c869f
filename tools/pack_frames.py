#!/usr/bin/env python3
"""Pack the frames a training run can touch into a store for the 'resident' wire format (cfg.data.wire = "resident",
tripled_amd/resident.py).

Walks the split lists of the config, collects every frame a sample can read -- the centre frame, each integer frame id's neighbour, the
other side when 's' is a frame id --, decodes each ONCE with the dataset's own decoder in worker processes and writes

  DIR/store.bin   planar uint8 [3,h,w] per frame, native size, rows tight, each frame on a 16-byte boundary
  DIR/store.json  format version, image extension, the sizes found, per frame (relative path, h, w, byte offset), total bytes

Packing the same tree again gives identical files.  A frame whose size cfg.data.raw_sizes does not list is an error.  Validation
datasets can use the wire only if 'val' was packed too (the default).

  python tools/pack_frames.py --config config/cfg_kitti_tripleD.py --out /data/kitti_store [--which train val] [--workers N]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--config", required=True)
    p.add_argument("--out", required=True, help="store directory (created)")
    p.add_argument("--which", nargs="+", default=["train", "val"], choices=["train", "val"])
    p.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1), help="decoder processes (0: decode in this process)")
    args = p.parse_args()
    import tripled_amd  # noqa: F401
    from mmcv import Config
    from tripled_amd import resident
    cfg = Config.fromfile(args.config)
    info = resident.pack_from_config(cfg.data, args.out, which=tuple(args.which), workers=args.workers)
    print("packed %d frames, %d bytes (%.2f GB), sizes %s, in %.1f s with %d workers -> %s"
          % (info["frames"], info["bytes"], info["bytes"] / 2 ** 30, info["raw_sizes"], info["seconds"], args.workers, args.out))


if __name__ == "__main__":
    main()
