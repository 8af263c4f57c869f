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

The 'resident' wire format is measured beside 'raw_u8' in the same run: the tree is packed
(tools/pack_frames.py's packer; time, size), the dataset is timed in one process and through the loader (with ``--workers`` and with 2
workers), the store is loaded onto the device (time), and expand_device_batch / td_lanczos_resize_u8_indexed are timed on the same frames
as the 'raw_u8' expansion.  ``--epoch-frames N`` adds what section 17 left open: one epoch of train.py -- the real loader, the real
Runner, config/cfg_kitti_tripleD.py -- over a fabricated tree of N KITTI-sized frames, in a child process per wire, img/s from the
logged iteration times after the capture.

  python tools/loader_bench.py [--ext png jpg] [--workers 8] [--samples 48] [--host-only] [--out profiles/loader/x.txt]
                               [--epoch-frames 2400 --epoch-workers 16 2]
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
WIRES = ("float32", "uint8", "raw_u8", "resident")
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


def dataset(root, files, ext, wire, store=None):
    from mono.datasets.kitti_dataset import KITTIRAWDataset
    return KITTIRAWDataset(root, files, H, W, list(FRAMES), cfg=ConfigDict(wire=wire, store=store), is_train=True, img_ext=ext)


def pack_tree(root, files, ext, store, workers, out):
    """Pack the tree for the 'resident' wire; one line of figures."""
    from tripled_amd import resident
    info = resident.pack([dataset(root, files, ext, "raw_u8")], store, workers=workers)
    out.append("pack %s: %d frames, %.1f MB (%.3f MB per frame) in %.2f s with %d decoder processes = %.1f frames/s"
               % (ext, info["frames"], info["bytes"] / 1e6, info["bytes"] / 1e6 / info["frames"], info["seconds"], workers,
                  info["frames"] / info["seconds"]))
    return info


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
    out.append("%-5s %-8s %14s %22s %16s %10s %10s" % ("ext", "wire", "one process", "%d workers (B=%d)" % (args.workers, B), "2 workers",
                                                       "vs uint8", "vs raw_u8"))
    rows, packs = {}, {}
    with tempfile.TemporaryDirectory() as root:
        for ext in args.ext:
            ext = "." + ext.lstrip(".")
            files = write_tree(os.path.join(root, ext[1:]), ext, args.frames)
            store = os.path.join(root, "store_" + ext[1:])
            pack_lines = []
            packs[ext] = pack_tree(os.path.join(root, ext[1:]), files, ext, store, args.pack_workers, pack_lines)
            for wire in WIRES:
                ds = dataset(os.path.join(root, ext[1:]), files, ext, wire, store)
                # the resident samples cost microseconds: more of them, or the timer's resolution is the result
                single = one_process(ds, args.samples * (50 if wire == "resident" else 1))
                more = 8 if wire == "resident" else 1
                multi = through_loader(ds, args.workers, args.batches * more) if args.workers > 0 else None
                two = through_loader(ds, 2, args.batches * more) if wire in ("raw_u8", "resident") else None
                rows[(ext, wire)] = (single, multi, two)
                print("[loader_bench] %s %s done" % (ext, wire), file=sys.stderr, flush=True)
            for wire in WIRES:
                single, multi, two = rows[(ext, wire)]

                def rel(base):
                    return "%.2fx" % (single / base[0]) + ("" if multi is None else " / %.2fx" % (multi / base[1]))
                out.append("%-5s %-8s %14.1f %22s %16s %10s %10s" % (ext, wire, single, "not measured" if multi is None else "%.1f" % multi,
                                                                   "not measured" if two is None else "%.1f" % two,
                                                                   rel(rows[(ext, "uint8")]), rel(rows[(ext, "raw_u8")])))
            out.extend(pack_lines)
    return {"rows": {"%s %s" % k: v for k, v in rows.items()}, "pack": packs}


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
    result = {"expand_uint8_us": t_u8, "expand_raw_u8_us": t_raw, "kernel_us": t_k, "floor_us": floor_us, "h2d_raw": h2d_raw, "h2d_u8": h2d_u8,
              "stage_uint8_ms": s_u8, "stage_raw_u8_ms": s_raw}
    result["resident"] = resident_device_part(args, out, dev)
    return result


def collate(samples):
    return {k: torch.stack([torch.as_tensor(s[k]) for s in samples]) for k in samples[0]}


def resident_device_part(args, out, dev):
    """The same B x 3 frames of a packed tree under 'resident' and under 'raw_u8': the expansion, the resize alone, the staging."""
    from mono.datasets import DevicePrefetcher, expand_device_batch
    from mono.datasets.raw_wire import KITTI_RAW_SIZES
    from tripled_amd import resident, resize
    with tempfile.TemporaryDirectory() as root:
        files = write_tree(root, ".png", max(args.frames, B + 2))
        store_dir = os.path.join(root, "store")
        pack_tree(root, files, ".png", store_dir, args.pack_workers, out)
        store = resident.get_store(store_dir, dev)
        out.append("store load: %.1f MB onto %s in %.3f s through two pinned buffers of at most %d MB = %.2f GB/s (the file was just "
                   "written: it comes from the page cache)" % (store.nbytes / 1e6, dev, store.load_seconds, resident.STAGING_BYTES >> 20,
                                                               store.nbytes / 1e9 / store.load_seconds))
        hosts = {}
        for wire in ("resident", "raw_u8"):
            ds = dataset(root, files, ".png", wire, store_dir)
            random.seed(1)
            torch.manual_seed(1)
            hosts[wire] = collate([ds[i] for i in range(B)])
    pf = DevicePrefetcher([], dev)
    staged = {w: pf._stage(b) for w, b in hosts.items()}
    torch.cuda.synchronize()
    a, b = expand_device_batch(dict(staged["resident"])), expand_device_batch(dict(staged["raw_u8"]))
    same = all(torch.equal(a[k], b[k]) for k in a)
    t_res = event_us(lambda: expand_device_batch(dict(staged["resident"])), args.rounds, args.inner)
    t_raw = event_us(lambda: expand_device_batch(dict(staged["raw_u8"])), args.rounds, args.inner)
    bank = resize.get_bank(KITTI_RAW_SIZES, H, W, dev)
    offsets = torch.cat([staged["resident"][("res_off", f)] for f in FRAMES])
    meta3 = staged["resident"]["raw_meta"].repeat(len(FRAMES), 1)
    canv = torch.cat([staged["raw_u8"][("raw_u8", f)] for f in FRAMES], 0)
    t_ki = event_us(lambda: resident.resize_from_store_hip(store, offsets, meta3, bank), args.rounds, args.inner)
    t_kc = event_us(lambda: resize.lanczos_resize_hip(canv, meta3, bank), args.rounds, args.inner)
    resize.check_banks()
    out.append("the same %d x %d frames of %dx%d from the packed tree, both wires (outputs bit-equal: %s)" % (B, len(FRAMES), H0, W0, same))
    out.append("expand_device_batch  wire=resident %8.1f (%.1f)" % t_res)
    out.append("expand_device_batch  wire=raw_u8   %8.1f (%.1f)   resident - raw_u8: %+.1f us" % (t_raw + (t_res[0] - t_raw[0],)))
    out.append("td_lanczos_resize_u8_indexed alone %8.1f (%.1f)" % t_ki)
    out.append("td_lanczos_resize_u8 alone         %8.1f (%.1f)   indexed - canvas: %+.1f us" % (t_kc + (t_ki[0] - t_kc[0],)))
    nbytes = {w: sum(v.numel() * v.element_size() for v in hosts[w].values()) for w in hosts}
    out.append("bytes per batch from the loader (all entries): resident %d (%.1f per sample), raw_u8 %.1f MB"
               % (nbytes["resident"], nbytes["resident"] / B, nbytes["raw_u8"] / 1e6))
    s_res, s_raw = stage_ms(hosts["resident"], dev, args.rounds), stage_ms(hosts["raw_u8"], dev, args.rounds)
    out.append("DevicePrefetcher staging of one pageable batch (pin + copy), wall ms, median (min): resident %.3f (%.3f), raw_u8 %.2f (%.2f)"
               % (s_res + s_raw))
    resident.release(store_dir)
    return {"expand_resident_us": t_res, "expand_raw_u8_us": t_raw, "indexed_kernel_us": t_ki, "canvas_kernel_us": t_kc,
            "bit_equal": same, "load_s": store.load_seconds, "store_bytes": store.nbytes, "stage_resident_ms": s_res, "stage_raw_u8_ms": s_raw}


# ---- one epoch of train.py, fed by the real loader ------------------------------------------------------------------------------------

def write_epoch_tree(root, n, distinct=24):
    """n KITTI-sized .png files cycling through ``distinct`` images (a decoder does not care that file 24 repeats file 0), and the split
    lists of one drive."""
    import shutil
    write_tree(root, ".png", distinct)
    d = os.path.join(root, DRIVE, "image_02/data")
    for i in range(distinct, n):
        shutil.copyfile(os.path.join(d, "%010d.png" % (i % distinct)), os.path.join(d, "%010d.png" % i))
    os.makedirs(os.path.join(root, "splits", "exp"))
    with open(os.path.join(root, "splits", "exp", "train_files.txt"), "w") as f:
        f.write("\n".join("%s %d l" % (DRIVE, i) for i in range(1, n - 1)) + "\n")


def epoch_part(args, out):
    import subprocess
    from mmcv import Config
    from mmcv.config import _unwrap
    from tripled_amd import resident
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = _unwrap(Config.fromfile(os.path.join(repo, "config", "cfg_kitti_tripleD.py"))._cfg_dict)
    result = {}
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        write_epoch_tree(root, args.epoch_frames)
        out.append("one epoch of train.py (config/cfg_kitti_tripleD.py: B = %d, %dx%d, frames %s; validate off, syncbn off, MIOpen immediate "
                   "mode, no tuned find-db) over %d KITTI-sized .png frames (tree written in %.1f s)"
                   % (B, H, W, list(FRAMES), args.epoch_frames, time.perf_counter() - t0))
        store = os.path.join(root, "store")
        info = resident.pack_from_config(ConfigDict(dict(base["data"], in_path=root, split_dir=os.path.join(root, "splits"), wire="raw_u8")),
                                         store, which=("train",), workers=args.pack_workers)
        out.append("pack: %d frames, %.2f GB in %.1f s with %d decoder processes = %.1f frames/s"
                   % (info["frames"], info["bytes"] / 1e9, info["seconds"], args.pack_workers, info["frames"] / info["seconds"]))
        out.append("%-9s %8s %12s %16s %16s %12s" % ("wire", "workers", "iterations", "time ms/iter", "data_time ms", "img/s"))
        runs = [("raw_u8", w) for w in args.epoch_workers] + [("resident", w) for w in (0, 2)]
        for wire, workers in runs:
            cfg = dict(base)
            cfg["data"] = dict(base["data"], in_path=root, split_dir=os.path.join(root, "splits"), gt_depth_path=None, wire=wire, store=store)
            cfg.update(validate=False, syncbn=False, total_epochs=1, workers_per_gpu=workers, cudnn_benchmark=False,
                       log_config=dict(interval=10, hooks=[dict(type="TextLoggerHook")]))
            cfg["lr_config"] = dict(cfg["lr_config"], warmup_iters=5)
            cfg_path = os.path.join(root, "cfg_%s_%d.json" % (wire, workers))
            with open(cfg_path, "w") as f:
                json.dump(cfg, f)
            work = os.path.join(root, "work_%s_%d" % (wire, workers))
            t0 = time.perf_counter()
            proc = subprocess.run([sys.executable, os.path.join(repo, "train.py"), "--config", cfg_path, "--work_dir", work, "--launcher", "none",
                                   "--gpus", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.epoch_timeout)
            wall = time.perf_counter() - t0
            if proc.returncode != 0:
                out.append("%-9s %8d   train.py failed (exit %d): %s" % (wire, workers, proc.returncode, proc.stdout[-400:].replace("\n", " | ")))
                if proc.returncode < 0 or proc.returncode in (124, 134, 137, 139):
                    out.append("a fault or a kill: no further epoch is started")
                    break
                continue
            logs = sorted(p for p in os.listdir(work) if p.endswith(".log.json"))
            rows = [json.loads(line) for line in open(os.path.join(work, logs[-1]))]
            rows = [r for r in rows if r.get("mode") == "train" and "time" in r and r.get("iter", 0) > 20]      # after warm-up and capture
            t = statistics.mean(r["time"] for r in rows)
            dt = statistics.mean(r.get("data_time", 0.0) for r in rows)
            out.append("%-9s %8d %12d %16.2f %16.2f %12.1f   (process wall %.1f s)"
                       % (wire, workers, (args.epoch_frames - 2) // B, t * 1e3, dt * 1e3, B / t, wall))
            result["%s %d" % (wire, workers)] = {"time_s": t, "data_time_s": dt, "img_s": B / t, "wall_s": wall, "log_rows": len(rows)}
            print("[loader_bench] epoch %s %d done" % (wire, workers), file=sys.stderr, flush=True)
    return result


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
    p.add_argument("--pack-workers", type=int, default=min(16, os.cpu_count() or 1), help="decoder processes of the packer")
    p.add_argument("--epoch-frames", type=int, default=0, help="frames of the tree one train.py epoch runs over (0: not measured)")
    p.add_argument("--epoch-workers", type=int, nargs="+", default=[16], help="loader workers of the raw_u8 epoch(s)")
    p.add_argument("--epoch-timeout", type=int, default=420, help="seconds one train.py child may take")
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
        if args.epoch_frames > 0:
            result["epoch"] = epoch_part(args, out)
        else:
            out.append("one epoch of train.py: not measured (--epoch-frames 0)")
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
