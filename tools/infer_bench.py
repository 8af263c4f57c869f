#!/usr/bin/env python3
"""Timing of the depth-inference path (tripled_amd.infer) on one GPU.

  1. the three kernels of csrc/td_infer.hip against the torch-op compositions they replace (the host statements of
     tripled_amd.infer run on the device), KITTI frame 375 x 1242 <-> network 192 x 640, B = 1 and 12: HIP events around
     ``--inner`` back-to-back calls, median over ``--rounds`` rounds, after a warm-up;
  2. images/s of DepthPredictor.predict (uint8 frames on the host in, disparity and depth on the device out) in fp32 and in
     bf16, wall clock with a device synchronisation per call, median over rounds;
  3. the same images through the loop body of scripts/eval_depth.evaluate, the only way to a disparity before the predictor:
     float conversion on the host, upload, fp32 eval forward, disp_to_depth, copy back, numpy resize_bilinear.
Model: cfg_kitti_tripleD (ResNet50 depth encoder), random weights.  Nothing is tuned per side: both run what the product runs.

  python tools/infer_bench.py [--rounds 20] [--inner 20] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tripled_amd  # noqa: F401,E402
from tripled_amd import infer  # noqa: E402

H0, W0, H, W = 375, 1242, 192, 640


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


def wall_ms(fn, rounds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(samples), min(samples)


def frames(B, seed=0):
    g = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, H0), np.linspace(0, 1, W0), indexing="ij")
    out = np.empty((B, H0, W0, 3), np.uint8)
    for i in range(B):
        for c in range(3):
            f = 127.5 + 100 * np.sin(6.28 * (g.uniform(1, 4) * y + g.uniform(1, 4) * x)) + g.uniform(-25, 25, (H0, W0))
            out[i, :, :, c] = np.clip(np.round(f), 0, 255)
    return out


def colorize_torch(x, vmin, vmax, lut):
    t = torch.floor(((x - vmin.view(-1, 1, 1)) / (vmax - vmin).view(-1, 1, 1)) * 256.0)
    return lut[t.clamp_(0, 255).long()]


def stage_rows(rounds, inner):
    dev = torch.device("cuda", 0)
    rows = []
    for B in (1, 12):
        img = torch.from_numpy(frames(B)).to(dev)
        for mirror in (False, True):
            k = event_us(lambda: infer.preprocess_hip(img, H, W, mirror), rounds, inner)
            t = event_us(lambda: infer.preprocess_torch(img, H, W, mirror), rounds, inner)
            rows.append(dict(stage="preprocess", B=B, flip=mirror, kernel_us=k[0], kernel_min_us=k[1], torch_us=t[0], torch_min_us=t[1]))
        for paired in (False, True):
            for dtype in (torch.float32, torch.bfloat16):
                net = torch.rand(B * (2 if paired else 1), 1, H, W, device=dev).to(dtype)
                k = event_us(lambda: infer.postprocess_hip(net, H0, W0, paired), rounds, inner)
                t = event_us(lambda: infer.postprocess_torch(net, H0, W0, paired), rounds, inner)
                rows.append(dict(stage="postprocess " + str(dtype).replace("torch.", ""), B=B, flip=paired, kernel_us=k[0],
                                 kernel_min_us=k[1], torch_us=t[0], torch_min_us=t[1]))
        disp = torch.rand(B, H0, W0, device=dev)
        vmin, vmax = disp.reshape(B, -1).amin(1), torch.full((B,), 0.95, device=dev)
        lut = infer._device_lut(dev)
        k = event_us(lambda: infer.colorize_hip(disp, vmin, vmax), rounds, inner)
        t = event_us(lambda: colorize_torch(disp, vmin, vmax, lut), rounds, inner)
        rows.append(dict(stage="colorize", B=B, flip=False, kernel_us=k[0], kernel_min_us=k[1], torch_us=t[0], torch_min_us=t[1]))
    return rows


def eval_loop_body(model, sample, dev):
    """scripts/eval_depth.evaluate, one iteration (sample: float32 [3,H,W] on the host, as the dataset returns it)."""
    from mono.core.evaluation import disp_to_depth
    from mono.core.evaluation.eval_hooks import resize_bilinear
    with torch.no_grad():
        batch = {k: torch.as_tensor(v).float().unsqueeze(0).to(dev) for k, v in sample.items()}
        scaled, _ = disp_to_depth(model(batch)[("disp", 0, 0)].float(), 0.1, 100)
        return resize_bilinear(scaled.cpu()[0, 0].numpy(), H0, W0)


def predict_rows(rounds):
    from mmcv import Config
    from mono.model import MONO
    dev = torch.device("cuda", 0)
    cfg = Config.fromfile(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "cfg_kitti_tripleD.py"))
    cfg.model["imgs_per_gpu"] = 1
    torch.manual_seed(0)
    model = MONO.module_dict[cfg.model["name"]](cfg.model).to(dev).eval()
    rows = []
    imgs = frames(12, seed=1)
    # the validation dataset's frames: resized to the network size on the host, float [3,H,W] in [0,1]
    net_size = infer.preprocess_torch(imgs, H, W).numpy()
    samples = [{("color", 0, 0): f, ("color_aug", 0, 0): f} for f in net_size]

    def baseline():
        for s in samples:
            eval_loop_body(model, s, dev)

    ms = wall_ms(baseline, max(3, rounds // 4))
    rows.append(dict(path="eval_depth loop body (fp32, one frame at a time)", B=1, ms_per_call=ms[0] / 12, imgs_per_s=12e3 / ms[0],
                     best_imgs_per_s=12e3 / ms[1]))
    for precision in ("fp32", "bf16"):
        for post in (False, True):
            p = infer.DepthPredictor(model, H, W, dev, precision=precision, post_process=post)
            for B in (1, 12):
                batch = imgs[:B]
                ms = wall_ms(lambda: p.predict(batch), rounds)
                rows.append(dict(path="DepthPredictor.predict %s%s" % (precision, " + flip post-processing" if post else ""), B=B,
                                 ms_per_call=ms[0], imgs_per_s=B * 1e3 / ms[0], best_imgs_per_s=B * 1e3 / ms[1]))
            del p
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--stages-only", action="store_true")
    args = ap.parse_args()
    stages = stage_rows(args.rounds, args.inner)
    print("%-22s %3s %5s %12s %12s %8s" % ("stage (375x1242<->192x640)", "B", "flip", "kernel us", "torch ops us", "ratio"))
    for r in stages:
        print("%-22s %3d %5s %12.1f %12.1f %8.2f" % (r["stage"], r["B"], "yes" if r["flip"] else "no", r["kernel_us"], r["torch_us"],
                                                     r["torch_us"] / r["kernel_us"]))
    preds = [] if args.stages_only else predict_rows(args.rounds)
    if preds:
        print("\n%-58s %3s %12s %10s" % ("path", "B", "ms per call", "imgs/s"))
        for r in preds:
            print("%-58s %3d %12.2f %10.1f" % (r["path"], r["B"], r["ms_per_call"], r["imgs_per_s"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(stages=stages, predict=preds, rounds=args.rounds, inner=args.inner), f, indent=1)


if __name__ == "__main__":
    main()
