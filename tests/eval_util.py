"""Shared pieces of the evaluation tests (test_eval_cpu.py, test_hip_eval.py): synthetic disparities with sparse ground truth, the
oracle per image with its per-pixel ratios, the float64 evaluation that measures the float32 host path's own noise, and the bounds.

Bounds of a row [abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, scale] against oracle.metrics.eval_single:
  * scale and the four error metrics: max(10 * e32, 1e-5 * |value|), e32 = |float32 host path - float64 evaluation| of the same
    inputs, computed on the spot; 1e-5 is the per-pixel depth bound of tests/test_hip_infer.py, the factor 10 allows for a
    different order of the same float32 roundings;
  * a1..a3: n_band / N + 1e-6, n_band = reference pixels whose ratio lies within relative 1e-5 of the threshold (a pixel that a
    rounding may carry across it); n_band / N <= 1e-3 is asserted on the reference alone."""
import numpy as np
import torch

from oracle import metrics as oracle_metrics
from tests.infer_util import smooth_disp

AFFINE = (9.99, 0.01)                  # disp_to_depth(., 0.1, 100): scaled = 0.01 + 9.99 disp
MIXED_SIZES = [(37, 53), (24, 40), (30, 61)]
KITTI_SIZES = [(375, 1242), (370, 1226), (374, 1238), (376, 1241)]
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3", "scale")


def scaled_disparity(disp):
    """float32 tensor [..] -> 0.01 + 9.99 disp as float32 numpy (the affine in float32, product and sum rounded separately)."""
    a, b = AFFINE
    return (b + a * disp.to(torch.float32)).numpy()


def sparse_gt(seed, disp_plane, gt_h, gt_w, density=0.3):
    """Ground truth for a disparity plane [h,w] (float32 tensor): about ``density`` of the entries non-zero, a scaled, noisy
    copy of the predicted depth there (so that the thresholds a1..a3 separate pixels); some entries exceed 80 and drop out."""
    g = np.random.default_rng(seed)
    depth = 1.0 / oracle_metrics.resize_bilinear(scaled_disparity(disp_plane), gt_h, gt_w).astype(np.float64)
    gt = depth * 7.3 * np.exp(0.25 * g.standard_normal((gt_h, gt_w)))
    gt[g.random((gt_h, gt_w)) >= density] = 0.0
    return gt.astype(np.float32)


def make_case(seed, sizes, h, w, dtype=torch.float32, density=0.3):
    """(disp [B,h,w] of ``dtype``, [gt_0, ...]); the ground truth follows the disparity as rounded to ``dtype``."""
    disp = smooth_disp(seed, len(sizes), h, w)[:, 0].to(dtype)
    gts = [sparse_gt(seed * 31 + i, disp[i].float(), gh, gw, density) for i, (gh, gw) in enumerate(sizes)]
    return disp, gts


def _mask(gt):
    gt_h, gt_w = gt.shape
    mask = np.logical_and(gt > 1e-3, gt < 80.0)
    crop = np.array([0.40810811 * gt_h, 0.99189189 * gt_h, 0.03594771 * gt_w, 0.96405229 * gt_w]).astype(np.int32)
    inside = np.zeros(mask.shape, bool)
    inside[crop[0]:crop[1], crop[2]:crop[3]] = True
    return np.logical_and(mask, inside)


def _resize_f64(img, out_h, out_w):
    in_h, in_w = img.shape

    def axis(n_out, n_in):
        s = (np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5
        i0 = np.floor(s).astype(np.int64)
        return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), s - i0

    y0, y1, ly = axis(out_h, in_h)
    x0, x1, lx = axis(out_w, in_w)
    img = img.astype(np.float64)
    rows = img[y0] * (1 - ly)[:, None] + img[y1] * ly[:, None]
    return rows[:, x0] * (1 - lx)[None] + rows[:, x1] * lx[None]


def eval_f64(scaled, gt, stereo):
    """The protocol with every step after the float32 inputs in float64: [8]."""
    mask = _mask(gt)
    pd = (1.0 / _resize_f64(scaled, *gt.shape))[mask]
    gd = gt.astype(np.float64)[mask]
    ratio = np.median(gd) / np.median(pd)
    pd = np.clip(pd * (36.0 if stereo else ratio), 1e-3, 80.0)
    return np.array(oracle_metrics.compute_errors(gd, pd) + (ratio,), dtype=np.float64)


class Reference:
    """oracle.metrics.eval_single of one image, with what the bounds need."""

    def __init__(self, scaled, gt, stereo):
        errors, ratio = oracle_metrics.eval_single(scaled, gt, stereo_scale=stereo)
        mask = _mask(gt)
        self.N = int(mask.sum())
        pd = (1.0 / oracle_metrics.resize_bilinear(scaled, *gt.shape))[mask]
        gd = gt[mask]
        self.scale = np.float32(np.median(gd) / np.median(pd))
        pd = np.clip(pd * (36.0 if stereo else self.scale), 1e-3, 80.0)
        assert oracle_metrics.compute_errors(gd, pd) == errors                 # the same statements: the same numbers
        self.row = np.array([float(v) for v in errors] + [float(self.scale)], dtype=np.float64)
        from mono.core.evaluation import evaluate_disparity
        host = evaluate_disparity(scaled, gt, stereo)
        host = np.array([host[k] for k in NAMES], dtype=np.float64)
        self.e32 = np.abs(host - eval_f64(scaled, gt, stereo))
        pix = np.maximum(gd / pd, pd / gd).astype(np.float64)
        self.n_band = np.array([int((np.abs(pix - t) <= 1e-5 * t).sum()) for t in THRESHOLDS])
        self.bound = np.maximum(10.0 * self.e32, 1e-5 * np.abs(self.row))
        self.bound[4:7] = self.n_band / max(self.N, 1) + 1e-6

    def band_ok(self):
        return bool((self.n_band <= 1e-3 * self.N).all())


def check_rows(rows, counts, refs, what):
    """rows [B,8], counts [B] (numpy) against one Reference per image; prints the measured deviations before asserting."""
    worst = np.zeros(8)
    for i, ref in enumerate(refs):
        assert ref.band_ok(), "%s image %d: %s of %d reference pixels lie on a threshold -- choose another seed" % (what, i, ref.n_band, ref.N)
        assert int(counts[i]) == ref.N, "%s image %d: count %d, reference %d" % (what, i, counts[i], ref.N)
        dev = np.abs(rows[i].astype(np.float64) - ref.row)
        worst = np.maximum(worst, dev / ref.bound)
        print("%s image %d (N %d): " % (what, i, ref.N) + "  ".join("%s %.2e/%.2e" % (n, d, b) for n, d, b in zip(NAMES, dev, ref.bound)))
    assert (worst <= 1.0).all(), "%s: deviation / bound = %s" % (what, dict(zip(NAMES, worst.round(3))))


class ListDataset(torch.utils.data.Dataset):
    """A validation dataset in the test: frames at network size with ground truths of mixed sizes."""

    def __init__(self, seed, n, h, w, sizes, wire="float32"):
        from tests.infer_util import smooth_image
        frames = smooth_image(seed, h, w, batch=n)                                  # uint8 [n,h,w,3]
        g = np.random.default_rng(seed)
        self.samples = []
        for i in range(n):
            gh, gw = sizes[i % len(sizes)]
            gt = (1.0 + 40.0 * g.random((gh, gw))).astype(np.float32)
            gt[g.random((gh, gw)) >= 0.3] = 0.0
            u8 = torch.from_numpy(frames[i]).permute(2, 0, 1).contiguous()
            if wire == "uint8":
                s = {("color_u8", 0): u8, "aug": torch.zeros(9)}
            else:
                img = u8.float().div(255.0)
                s = {("color", 0, 0): img, ("color_aug", 0, 0): img.clone()}
            s["gt_depth"] = gt
            self.samples.append(s)

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        return dict(self.samples[i])


def frame_references(model, dataset, device, stereo, disps=None):
    """One Reference per frame from the model's batch-1 forward (scripts/eval_depth.evaluate's), or from ``disps``."""
    from mono.core.evaluation import disp_to_depth
    refs = []
    with torch.no_grad():
        for i in range(len(dataset)):
            s = dataset[i]
            if disps is None:
                batch = {k: torch.as_tensor(v).float().unsqueeze(0).to(device) for k, v in s.items() if k != "gt_depth"}
                scaled = disp_to_depth(model(batch)[("disp", 0, 0)].float(), 0.1, 100)[0].cpu()[0, 0].numpy()
            else:
                scaled = disp_to_depth(disps[i].float().cpu(), 0.1, 100)[0].numpy()
            refs.append(Reference(scaled, np.asarray(s["gt_depth"], np.float32), stereo))
    return refs


def check_mean(mean, scales, refs, what, want=None, want_scales=None):
    """DepthEvaluator's (mean dict, scales) against the frames' references (or against ``want`` / ``want_scales``, the host
    loop's, with the references' bounds): the mean of the per-frame bounds."""
    want = np.mean([r.row for r in refs], 0) if want is None else np.array([want[k] for k in NAMES[:7]] + [0.0])
    bound = np.mean([r.bound for r in refs], 0)
    for r in refs:
        assert r.band_ok()
    got = np.array([mean[k] for k in NAMES[:7]])
    dev = np.abs(got - want[:7])
    print("%s mean: " % what + "  ".join("%s %.2e/%.2e" % (n, d, b) for n, d, b in zip(NAMES, dev, bound)))
    assert (dev <= bound[:7]).all(), "%s: %s" % (what, dict(zip(NAMES, (dev / bound[:7]).round(3))))
    for i, r in enumerate(refs):
        target = r.row[7] if want_scales is None else float(want_scales[i])
        assert abs(float(scales[i]) - target) <= r.bound[7], "%s: scale of frame %d" % (what, i)
