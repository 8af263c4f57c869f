"""KITTI depth evaluation in batches: a validation dataset and a model in, the seven standard metrics out.

The protocol is mono.core.evaluation.eval_hooks.evaluate_disparity (reference scripts/eval_depth.py:73-101): resize the scaled
disparity to the ground-truth size by cv2's INTER_LINEAR definition, invert, keep min_depth < gt < max_depth inside the Garg crop,
scale by the ratio of the medians (x 36 for stereo), clamp, compute_errors.  The host path does it one frame at a time in numpy;
here a batch of frames with ground truths of different sizes is scored at once and the rows stay on the device until the end.

Three layers, as in infer.py:
  * ``evaluate_disparity_torch``: the protocol as plain torch statements on any device (float64 coordinate, float32
    interpolation).  It is the host path (``device='cpu'``) and what the kernel is tested against, alongside the oracle.
  * ``evaluate_disparity_hip`` / ``masked_median_hip``: csrc/td_eval.hip (td_eval_depth, td_masked_median).  Device tensors only;
    a CPU tensor is an error.
  * ``DepthEvaluator``: batches of a dataset -> forward -> (flip post-processing) -> scores, one copy to the host at the end.

Deviation from the host path: the interpolation is float32 where eval_hooks.resize_bilinear interpolates in float64 and rounds
once (DESIGN.md section 15 has the measured distance); the coordinate is float64 in both.
"""
import numpy as np
import torch

from . import infer, native, resize

METRICS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
COLUMNS = METRICS + ("scale",)
MIN_DEPTH = 1e-3
MAX_DEPTH = 80
STEREO_SCALE_FACTOR = native.CONSTANTS["TD_STEREO_SCALE_FACTOR"]


def garg_crop(gt_h, gt_w):
    """(y0, y1, x0, x1) of the Garg crop, the host path's expression (float64 products, truncated to int32)."""
    return np.array([0.40810811 * gt_h, 0.99189189 * gt_h, 0.03594771 * gt_w, 0.96405229 * gt_w]).astype(np.int32)


def pad_ground_truth(gt_list, device):
    """Ground truths of different sizes -> (gt float32 [B,Hmax,Wmax] zero-padded at the bottom and right, sizes int32 [B,2] =
    (gt_h, gt_w), crops int32 [B,4] = garg_crop), all on ``device``."""
    gts = [np.asarray(g.cpu() if torch.is_tensor(g) else g, dtype=np.float32) for g in gt_list]
    if not gts or any(g.ndim != 2 for g in gts):
        raise ValueError("gt_list: a non-empty list of 2-D depth maps")
    sizes = np.array([g.shape for g in gts], dtype=np.int32)
    crops = np.stack([garg_crop(int(h), int(w)) for h, w in sizes], 0)
    gt = np.zeros((len(gts), int(sizes[:, 0].max()), int(sizes[:, 1].max())), np.float32)
    for i, g in enumerate(gts):
        gt[i, :g.shape[0], :g.shape[1]] = g
    return torch.from_numpy(gt).to(device), torch.from_numpy(sizes).to(device), torch.from_numpy(crops).to(device)


def _as_planes(disp):
    if disp.dim() == 4 and disp.shape[1] == 1:
        disp = disp[:, 0]
    if disp.dim() != 3:
        raise ValueError("disp: [B,h,w] or [B,1,h,w], got %s" % (tuple(disp.shape),))
    return disp


def _affine(affine):
    return affine if affine is not None else infer.disp_to_depth_affine(0.1, 100.0)


# ---------------------------------------------------------------------------------------------------------------------------
# host statements

def _axis(n_out, n_in, device):
    s = (torch.arange(n_out, dtype=torch.float64, device=device) + 0.5) * (n_in / n_out) - 0.5
    f = torch.floor(s)
    lam = s - f
    i0 = f.to(torch.int64)
    return i0.clamp(0, n_in - 1), (i0 + 1).clamp(0, n_in - 1), (1.0 - lam).to(torch.float32), lam.to(torch.float32)


def resize_scaled_torch(scaled, out_h, out_w):
    """eval_hooks.resize_bilinear on a float32 [h,w] tensor: the coordinate in float64, the interpolation (rows, then columns)
    in float32."""
    y0, y1, wy0, wy1 = _axis(out_h, scaled.shape[0], scaled.device)
    x0, x1, wx0, wx1 = _axis(out_w, scaled.shape[1], scaled.device)
    rows = scaled[y0] * wy0[:, None] + scaled[y1] * wy1[:, None]
    return rows[:, x0] * wx0[None] + rows[:, x1] * wx1[None]


def median_torch(v):
    """np.median of a 1-D float32 tensor: 0.5 * (lower + upper) of the two middle values (torch.median returns the lower)."""
    n = v.numel()
    s = torch.sort(v).values
    return 0.5 * (s[(n - 1) // 2] + s[n // 2])


def evaluate_disparity_torch(disp, gt_list, stereo_scale=False, affine=None, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH):
    """disp: the network's sigmoid disparity [B,h,w] (or [B,1,h,w]), any float dtype; gt_list: B depth maps.
    Returns (float32 [B,8] = METRICS + scale, int32 [B] = pixels in the mask) on disp's device; an empty mask gives a NaN row."""
    disp = _as_planes(disp)
    a, b = _affine(affine)
    dev = disp.device
    rows, counts = [], []
    for d, g in zip(disp, gt_list):
        gt = torch.as_tensor(np.asarray(g.cpu() if torch.is_tensor(g) else g, dtype=np.float32)).to(dev)
        gt_h, gt_w = gt.shape
        pred = 1.0 / resize_scaled_torch(b + a * d.to(torch.float32), gt_h, gt_w)
        y0, y1, x0, x1 = (int(v) for v in garg_crop(gt_h, gt_w))
        mask = torch.zeros_like(gt, dtype=torch.bool)
        mask[y0:y1, x0:x1] = True
        mask &= (gt > min_depth) & (gt < max_depth)
        p, t = pred[mask], gt[mask]
        counts.append(p.numel())
        if p.numel() == 0:
            rows.append(torch.full((8,), float("nan"), dtype=torch.float32, device=dev))
            continue
        scale = median_torch(t) / median_torch(p)
        p = torch.clamp(p * (float(STEREO_SCALE_FACTOR) if stereo_scale else scale), min_depth, max_depth)
        ratio = torch.maximum(t / p, p / t)
        diff = t - p
        n = float(p.numel())
        rows.append(torch.stack([
            ((diff.abs() / t).double().sum() / n).float(),
            ((diff * diff / t).double().sum() / n).float(),
            torch.sqrt((diff * diff).double().sum() / n).float(),
            torch.sqrt(((torch.log(t) - torch.log(p)) ** 2).double().sum() / n).float(),
            ((ratio < 1.25).sum().double() / n).float(),
            ((ratio < 1.25 ** 2).sum().double() / n).float(),
            ((ratio < 1.25 ** 3).sum().double() / n).float(),
            scale.float()]))
    return torch.stack(rows, 0), torch.tensor(counts, dtype=torch.int32, device=dev)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels

def eval_workspace(B, Hmax, Wmax, device):
    """The scratch buffer of evaluate_disparity_hip for batches up to this shape (uint8, td_eval_depth_workspace_bytes)."""
    n = native.load().td_eval_depth_workspace_bytes(int(B), int(Hmax), int(Wmax))
    if n <= 0:
        raise native.NativeLibraryError("td_eval_depth_workspace_bytes(%d, %d, %d): unsupported shape" % (B, Hmax, Wmax))
    return torch.empty(n, dtype=torch.uint8, device=device)


def evaluate_disparity_hip(disp, gt, sizes, crops, stereo_scale=False, affine=None, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH,
                           workspace=None):
    """evaluate_disparity_torch as the launch chain of td_eval_depth.  disp: fp32 / bf16 [B,h,w] (or [B,1,h,w]); gt, sizes,
    crops: pad_ground_truth's, on the same HIP device.  No synchronisation: the results are device tensors."""
    lib = native.load()
    disp = _as_planes(disp)
    native.require_device(disp, gt, sizes, crops)
    if disp.dtype not in native.DTYPE_CODES:
        raise ValueError("disp: fp32 / bf16, got %s" % disp.dtype)
    B, h, w = disp.shape
    if gt.dim() != 3 or gt.shape[0] != B or gt.dtype != torch.float32:
        raise ValueError("gt: float32 [%d,Hmax,Wmax], got %s %s" % (B, tuple(gt.shape), gt.dtype))
    if tuple(sizes.shape) != (B, 2) or tuple(crops.shape) != (B, 4) or sizes.dtype != torch.int32 or crops.dtype != torch.int32:
        raise ValueError("sizes: int32 [B,2], crops: int32 [B,4]")
    a, b = _affine(affine)
    disp, gt, sizes, crops = disp.contiguous(), gt.contiguous(), sizes.contiguous(), crops.contiguous()
    Hmax, Wmax = gt.shape[1:]
    need = lib.td_eval_depth_workspace_bytes(B, Hmax, Wmax)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = eval_workspace(B, Hmax, Wmax, disp.device)
    metrics = torch.empty(B, 8, device=disp.device, dtype=torch.float32)
    counts = torch.empty(B, device=disp.device, dtype=torch.int32)
    native.call("td_eval_depth", disp, disp.dtype, B, h, w, a, b, gt, Hmax, Wmax, sizes, crops, min_depth, max_depth, bool(stereo_scale),
                workspace, workspace.numel() * workspace.element_size(), metrics, counts)
    return metrics, counts


def masked_median_hip(values):
    """float32 [B,n] on a HIP device, an entry <= 0 is absent -> (np.median of each row's present entries float32 [B] (NaN where
    there are none), their number int32 [B])."""
    lib = native.load()
    native.ptr(values)          # device and contiguous
    if values.dim() != 2 or values.dtype != torch.float32 or values.numel() == 0:
        raise ValueError("values: non-empty float32 [B,n], got %s %s" % (tuple(values.shape), values.dtype))
    B, n = values.shape
    need = lib.td_masked_median_workspace_bytes(B)
    workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=values.device)
    median = torch.empty(B, device=values.device, dtype=torch.float32)
    count = torch.empty(B, device=values.device, dtype=torch.int32)
    native.call("td_masked_median", values, B, n, workspace, workspace.numel(), median, count)
    return median, count


# ---------------------------------------------------------------------------------------------------------------------------

def _with_mirrored(batch):
    """Entries B..2B-1 = the horizontally mirrored frames (images: 4-D tensors); everything else is repeated."""
    return {k: torch.cat([v, v.flip(3) if v.dim() == 4 else v], 0) for k, v in batch.items()}


class DepthEvaluator:
    """evaluate(dataset) -> (mean of METRICS over the frames, per-frame median ratios): what scripts/eval_depth.evaluate returns.

    model         a depth model of this build: ``model(batch)[("disp", 0, 0)]``.  fp32 runs the caller's model where it stands
                  (its own copy if it lives on another device) and restores its training mode; bf16 runs the BatchNorm-folded
                  copy under autocast, as DepthPredictor does.  The caller's model is never moved or changed.
    device        'cuda[:i]': td_eval_depth scores each batch and the rows stay on the device; 'cpu': evaluate_disparity_torch
    post_process  the mirrored frames ride in the same batch and are blended at network size by td_disp_postprocess
                  (batch_post_process_disparity, reference scripts/eval_depth_pp.py)
    stereo_scale  x 36 instead of the median ratio (which is reported either way)
    """

    def __init__(self, model, device, batch_size=12, precision="fp32", post_process=False, stereo_scale=False):
        self.device = infer.check_precision(device, precision, batch_size)
        self.on_hip = self.device.type == "cuda"
        self.model = model
        self.batch_size = int(batch_size)
        self.precision = precision
        self.post_process = bool(post_process)
        self.stereo_scale = bool(stereo_scale)
        self._workspace = None
        self._velo_workspace = None

    def _forward(self, net, batch):
        if self.precision == "bf16":
            batch = {k: v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v for k, v in batch.items()}
        with infer.autocast_for(self.precision):
            return net(batch)[("disp", 0, 0)]

    def ground_truth(self, samples):
        """What score() takes for these samples: their "gt_depth" maps as a list, or, for samples that carry a raw scan instead
        (cfg.data.gt_source = "velodyne": "velo", "velo_P", "gt_size"), the maps made from the scans -- by td_velo_depth as the padded
        (gt, sizes, crops) on a HIP device, by the numpy statement as a list on the host."""
        if "velo" not in samples[0]:
            return [np.asarray(s["gt_depth"], dtype=np.float32) for s in samples]
        from . import velodyne
        if self.on_hip:
            sizes = np.array([[int(v) for v in s["gt_size"]] for s in samples])
            need = native.load().td_velo_depth_workspace_bytes(len(samples), int(sizes[:, 0].max()), int(sizes[:, 1].max()))
            if self._velo_workspace is None or self._velo_workspace.numel() < need:
                self._velo_workspace = velodyne.velo_workspace(max(len(samples), self.batch_size), sizes[:, 0].max(), sizes[:, 1].max(),
                                                               self.device)
        return velodyne.batch_ground_truth([s["velo"] for s in samples], [s["velo_P"] for s in samples],
                                           [s["gt_size"] for s in samples], self.device, workspace=self._velo_workspace)

    def score(self, disp_net, gt_list):
        """Network disparity [B*(1+post_process),1,h,w] + B ground truths (a list of maps, or the padded (gt, sizes, crops) of
        ground_truth) -> ([B,8], [B]) on the device."""
        h, w = disp_net.shape[2:]
        if self.on_hip:
            if self.post_process:
                disp_net = infer.postprocess_hip(disp_net, h, w, paired=True, want_depth=False)[0]
            gt, sizes, crops = gt_list if isinstance(gt_list, tuple) else pad_ground_truth(gt_list, self.device)
            need = native.load().td_eval_depth_workspace_bytes(gt.shape[0], gt.shape[1], gt.shape[2])
            if self._workspace is None or self._workspace.numel() < need:
                self._workspace = eval_workspace(max(gt.shape[0], self.batch_size), gt.shape[1], gt.shape[2], self.device)
            return evaluate_disparity_hip(disp_net, gt, sizes, crops, self.stereo_scale, workspace=self._workspace)
        if self.post_process:
            disp_net = infer.postprocess_torch(disp_net, h, w, paired=True)[0]
        return evaluate_disparity_torch(disp_net, gt_list, self.stereo_scale)

    def evaluate_rows(self, dataset, indices=None):
        """The [n,8] rows (METRICS + scale) and the [n] counts of the frames ``indices`` (default: all), as numpy arrays, after
        ONE copy to the host.  A frame whose mask is empty raises ValueError naming its index."""
        indices = list(range(len(dataset))) if indices is None else list(indices)
        if not indices:
            return np.zeros((0, 8), np.float32), np.zeros((0,), np.int32)
        from mono.datasets import collate_validation
        net, restore = infer.eval_network(self.model, self.device, self.precision)
        rows, counts = [], []
        with torch.no_grad(), restore:
            for at in range(0, len(indices), self.batch_size):
                samples = [dataset[i] for i in indices[at:at + self.batch_size]]
                gts = self.ground_truth(samples)
                batch = collate_validation(samples, self.device)
                if self.post_process:
                    batch = _with_mirrored(batch)
                m, c = self.score(self._forward(net, batch), gts)
                rows.append(m)
                counts.append(c)
        rows, counts = torch.cat(rows, 0).cpu().numpy(), torch.cat(counts, 0).cpu().numpy()          # the one copy
        if self.on_hip:
            resize.check_banks()          # 'raw_u8' wire format: a frame the resize kernel zero-filled raises here (no bank: no read)
        empty = np.nonzero(counts == 0)[0]
        if len(empty):
            raise ValueError("frame %d: no ground-truth pixel inside the crop and the depth range" % indices[int(empty[0])])
        return rows, counts

    def evaluate(self, dataset):
        rows, _ = self.evaluate_rows(dataset)
        mean = {k: float(np.mean(rows[:, j].astype(np.float64))) for j, k in enumerate(METRICS)}
        return mean, rows[:, 7].astype(np.float64)
