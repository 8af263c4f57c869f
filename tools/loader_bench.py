#!/usr/bin/env python3
"""What the 'raw_u8' wire format takes from the loader workers and what it adds to the device.

Host part (any machine): a temporary KITTI-shaped tree of 1242 x 375 frames (.png and .jpg) is written, and
KITTIRAWDataset.__getitem__ -- three frames, training mode -- is timed for the wires "float32", "uint8" and "raw_u8":
samples/s in one process, and through build_dataloader with ``--workers`` workers (at most 16).  The yardstick of the host
gain is the "uint8" wire in the same run on the same machine, which is recorded with the figures.

Device part (needs a GPU; ``--host-only`` skips it, and without a GPU it is reported as not measured):
  * expand_device_batch for B = 12 x 3 frames under "uint8" and under "raw_u8": HIP events around ``--inner`` back-to-back
    calls, median over ``--rounds`` rounds, after a warm-up;
  * td_lanczos_resize_u8 alone, next to its byte floor: (bytes read + bytes written) / the HBM peak bench.py's
    roofline.frac uses;
  * the host->device bytes per step of both wires, and what DevicePrefetcher's staging of one batch (pin + copy) takes.

  python tools/loader_bench.py [--ext png jpg] [--workers 8] [--samples 48] [--host-only] [--out profiles/loader/x.txt]
"""
import argparse
import json
import os
import platform
import random
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tripled_amd  # noqa: F401,E402
from mmcv import ConfigDict  # noqa: E402

H0, W0, H, W, B, FRAMES = 375, 1242, 192, 640, 12, (0, -1, 1)
HBM_PEAK_GBS = 8000.0        # bench.py: HBM_PEAK_GBS, the peak roofline.frac is computed against
WIRES = ("float32", "uint8", "raw_u8")
DRIVE = "2011_09_26/2011_09_26_drive_0001_sync"


def write_tree(root, ext, n):
    """n frames of smooth structure plus noise (a plain-noise PNG decodes unrepresentatively slowly)."""
    from PIL import Image
    d = os.path.join(root, DRIVE, "image_02/data")
    os.makedirs(d, exist_ok=True)
    g = np.random.default_rng(0)
    y, x = np.meshgrid(np.linspace(0, 1, H0), np.linspace(0, 1, W0), indexing="ij")
    for i in range(n):
        img = np.empty((H0, W0, 3), np.uint8)
        for c in range(3):
            f = 127.5 + 100 * np.sin(6.28 * (g.uniform(1, 4) * y + g.uniform(1, 4) * x)) + g.uniform(-25, 25, (H0, W0))
            img[:, :, c] = np.clip(np.round(f), 0, 255)
        Image.fromarray(img).save(os.path.join(d, "%010d%s" % (i, ext)), **({"quality": 92} if ext == ".jpg" else {}))
    return ["%s %d l" % (DRIVE, i) for i in range(1, n - 1)]


def dataset(root, files, ext, wire):
    from mono.datasets.kitti_dataset import KITTIRAWDataset
    return KITTIRAWDataset(root, files, H, W, list(FRAMES), cfg=ConfigDict(wire=wire), is_train=True, img_ext=ext)


def one_process(ds, n):
    random.seed(0)
    torch.manual_seed(0)
    ds[0]
    t0 = time.perf_counter()
    for i in range(n):
        ds[i % len(ds)]
    return n / (time.perf_counter() - t0)


def through_loader(ds, workers, n_batches):
    from mono.datasets import build_dataloader
    loader = build_dataloader(ds, B, workers, 1, dist=False, pin_memory=False)
    count, t0, seen = 0, None, 0
    while seen < n_batches + 1:
        for batch in loader:
            if t0 is None:                 # the first batch pays the workers' start
                t0 = time.perf_counter()
            else:
                count += int(batch["K"].shape[0])
            seen += 1
            if seen >= n_batches + 1:
                break
    rate = count / (time.perf_counter() - t0)
    del loader
    return rate


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def host_part(args, out):
    out.append("host: %s, %d CPUs visible, %s, torch %s, Pillow %s" % (cpu_model(), os.cpu_count() or 0, platform.platform(),
                                                                      torch.__version__, __import__("PIL").__version__))
    out.append("KITTIRAWDataset.__getitem__, frames %s, training mode, %dx%d -> %dx%d; samples/s" % (list(FRAMES), H0, W0, H, W))
    out.append("%-5s %-8s %14s %22s %10s" % ("ext", "wire", "one process", "%d workers (B=%d)" % (args.workers, B), "vs uint8"))
    rows = {}
    with tempfile.TemporaryDirectory() as root:
        for ext in args.ext:
            ext = "." + ext.lstrip(".")
            files = write_tree(os.path.join(root, ext[1:]), ext, args.frames)
            for wire in WIRES:
                ds = dataset(os.path.join(root, ext[1:]), files, ext, wire)
                single = one_process(ds, args.samples)
                multi = through_loader(ds, args.workers, args.batches) if args.workers > 0 else None
                rows[(ext, wire)] = (single, multi)
                print("[loader_bench] %s %s done" % (ext, wire), file=sys.stderr, flush=True)
            for wire in WIRES:
                single, multi = rows[(ext, wire)]
                base = rows[(ext, "uint8")]
                rel = "%.2fx" % (single / base[0]) + ("" if multi is None else " / %.2fx" % (multi / base[1]))
                out.append("%-5s %-8s %14.1f %22s %10s" % (ext, wire, single, "not measured" if multi is None else "%.1f" % multi, rel))
    return {"%s %s" % k: v for k, v in rows.items()}


def event_us(fn, rounds, inner):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1) / inner * 1e3)
    return statistics.median(samples), min(samples)


def stage_ms(batch, dev, rounds):
    """DevicePrefetcher's staging of one pageable host batch -- pin_memory, the copy, the float cast of the small entries --
    as wall time to completion (in training it runs on a side stream under the previous step)."""
    from mono.datasets import DevicePrefetcher
    pf = DevicePrefetcher([], dev)
    samples = []
    for i in range(rounds + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pf._stage(batch)
        torch.cuda.synchronize()
        if i >= 2:
            samples.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(samples), min(samples)


def device_part(args, out):
    from mono.datasets import expand_device_batch
    from mono.datasets.raw_wire import KITTI_RAW_SIZES, canvas_of, raw_spec
    from tripled_amd import resize
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    sizes = KITTI_RAW_SIZES
    Hc, Wc = canvas_of(sizes)
    aug = torch.zeros(B, 9)
    aug[::2] = torch.tensor([1.0, 2, 0, 3, 1, 1.1, 0.9, 1.15, 0.05])
    meta = torch.stack([torch.arange(B) % len(sizes), torch.arange(B) % 2], 1).to(torch.int32)
    raw_host = {("raw_u8", f): torch.randint(0, 256, (B, 3, Hc, Wc), generator=g, dtype=torch.uint8) for f in FRAMES}
    raw_host.update({"aug": aug, "raw_meta": meta, "raw_spec": raw_spec(H, W, sizes).unsqueeze(0).repeat(B, 1)})
    u8_host = {("color_u8", f): torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8) for f in FRAMES}
    u8_host["aug"] = aug
    raw = {k: (v if k == "raw_spec" else v.to(dev)) for k, v in raw_host.items()}
    u8 = {k: v.to(dev) for k, v in u8_host.items()}
    bank = resize.get_bank(sizes, H, W, dev)
    stacked = torch.cat([raw[("raw_u8", f)] for f in FRAMES], 0)
    meta3 = meta.to(dev).repeat(len(FRAMES), 1)
    t_u8 = event_us(lambda: expand_device_batch(dict(u8)), args.rounds, args.inner)
    t_raw = event_us(lambda: expand_device_batch(dict(raw)), args.rounds, args.inner)
    t_k = event_us(lambda: resize.lanczos_resize_hip(stacked, meta3, bank), args.rounds, args.inner)
    n = B * len(FRAMES)
    read = sum(3 * sizes[int(i)][0] * sizes[int(i)][1] for i in meta[:, 0].tolist()) * len(FRAMES)
    written = n * 3 * H * W
    floor_us = (read + written) / (HBM_PEAK_GBS * 1e9) * 1e6
    out.append("device: %s, B = %d x %d frames, %d rounds of %d calls, median (min) in us" % (torch.cuda.get_device_name(0), B, len(FRAMES),
                                                                                          args.rounds, args.inner))
    out.append("expand_device_batch  wire=uint8   %9.1f (%.1f)" % t_u8)
    out.append("expand_device_batch  wire=raw_u8  %9.1f (%.1f)   added per step: %.1f us" % (t_raw + (t_raw[0] - t_u8[0],)))
    out.append("td_lanczos_resize_u8 alone        %9.1f (%.1f)   byte floor %.1f us = (%.1f MB read + %.1f MB written) / %.0f GB/s; "
               "%.1f x the floor" % (t_k + (floor_us, read / 1e6, written / 1e6, HBM_PEAK_GBS, t_k[0] / floor_us)))
    h2d_raw, h2d_u8 = n * 3 * Hc * Wc, n * 3 * H * W
    out.append("host->device bytes per step (frames): raw_u8 %.1f MB, uint8 %.1f MB" % (h2d_raw / 1e6, h2d_u8 / 1e6))
    s_u8, s_raw = stage_ms(u8_host, dev, args.rounds), stage_ms(raw_host, dev, args.rounds)
    out.append("DevicePrefetcher staging of one pageable batch (pin + copy), wall ms, median (min): uint8 %.2f (%.2f), raw_u8 %.2f (%.2f)"
               % (s_u8 + s_raw))
    return {"expand_uint8_us": t_u8, "expand_raw_u8_us": t_raw, "kernel_us": t_k, "floor_us": floor_us, "h2d_raw": h2d_raw, "h2d_u8": h2d_u8,
            "stage_uint8_ms": s_u8, "stage_raw_u8_ms": s_raw}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ext", nargs="+", default=["png", "jpg"])
    p.add_argument("--workers", type=int, default=8)
    p.add_argument("--frames", type=int, default=26, help="frames written per tree")
    p.add_argument("--samples", type=int, default=48, help="samples timed in one process, per wire")
    p.add_argument("--batches", type=int, default=8, help="batches of %d timed through the loader, per wire" % B)
    p.add_argument("--rounds", type=int, default=20)
    p.add_argument("--inner", type=int, default=20)
    p.add_argument("--host-only", action="store_true")
    p.add_argument("--device-only", action="store_true")
    p.add_argument("--out", default=None, help="also write the table here")
    p.add_argument("--json", default=None)
    args = p.parse_args()
    if not 0 <= args.workers <= 16:
        p.error("--workers must be 0..16")
    out, result = [], {}
    if not args.device_only:
        result["host"] = host_part(args, out)
    if args.host_only:
        out.append("device part: not measured (--host-only)")
    elif not torch.cuda.is_available():
        out.append("device part: not measured (no GPU on this machine)")
    else:
        result["device"] = device_part(args, out)
    text = "\n".join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1, default=str)


if __name__ == "__main__":
    main()
