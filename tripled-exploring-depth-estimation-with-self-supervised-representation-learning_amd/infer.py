"""Depth inference: a trained checkpoint and an image in, disparity, depth and the magma picture out.

The reference does this in three programs: scripts/infer.py (one image: ``transform`` resizes to the network size, ``predict``
resizes the disparity back and converts it to depth, ``plt.imsave`` writes the magma picture with vmax at the 95th
percentile), scripts/infer_singleimage.py (the same over the validation split) and scripts/eval_depth_pp.py
(``batch_post_process_disparity``: the prediction blended with the un-mirrored prediction of the mirrored image).

Three layers here:
  * ``preprocess_torch`` / ``postprocess_torch`` / ``colorize_numpy``: the formulas as plain torch / numpy statements.  They are
    the host path (``device='cpu'``) and what the kernels are tested against.
  * ``preprocess_hip`` / ``postprocess_hip`` / ``colorize_hip``: the same three stages as one launch each of
    csrc/td_infer.hip (td_infer_preprocess, td_disp_postprocess, td_colorize).  Device tensors only; a CPU tensor is an error.
  * ``DepthPredictor``: ``predict(images) == postprocess(forward(preprocess(images)))`` on either device, plus
    ``fold_batchnorm`` for the bf16 forward.

Nothing here imports matplotlib: the colour table is 256 rows of data (magma_lut.txt, next to this file).
"""
import collections
import contextlib
import copy
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import native

_LUT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "magma_lut.txt")
_lut_host = None
_lut_device = {}

# depth = depth_scale / (a * disp + b)
REFERENCE_AFFINE = (1.0 / 1e-3, 1.0 / 80)      # reference scripts/infer.py:21-23,43-45: MIN_DEPTH = 1e-3, MAX_DEPTH = 80 ...
REFERENCE_DEPTH_SCALE = 36.0                   # ... and SCALE = 36 (stereo baseline factor)

Prediction = collections.namedtuple("Prediction", ["disp", "depth", "disp_net"])


def disp_to_depth_affine(min_depth, max_depth):
    """(a, b) of the reference's disp_to_depth (layers.py): scaled = 1/max + (1/min - 1/max) * disp, depth = 1 / scaled."""
    return 1.0 / min_depth - 1.0 / max_depth, 1.0 / max_depth


def magma_lut():
    """matplotlib's 'magma' as uint8 [256, 3] (matplotlib.colormaps['magma'](np.arange(256), bytes=True)[:, :3])."""
    global _lut_host
    if _lut_host is None:
        lut = np.loadtxt(_LUT_PATH, dtype=np.uint8)
        assert lut.shape == (256, 3) and lut.dtype == np.uint8
        _lut_host = lut
    return _lut_host


# ---------------------------------------------------------------------------------------------------------------------------
# host statements

def _as_batch(images, device=None):
    """list of H x W x 3 uint8 arrays / one array / [B,H,W,3] array or tensor -> uint8 tensor [B,H,W,3]."""
    if isinstance(images, (list, tuple)):
        images = torch.stack([torch.from_numpy(np.array(i)) if not torch.is_tensor(i) else i for i in images], 0)
    elif not torch.is_tensor(images):
        images = torch.from_numpy(np.array(images))
    if images.dim() == 3:
        images = images.unsqueeze(0)
    if images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8:
        raise ValueError("images: same-sized H x W x 3 uint8 arrays, got %s %s" % (tuple(images.shape), images.dtype))
    if device is not None:
        images = images.to(device)
    return images.contiguous()


def preprocess_torch(images, height, width, mirror=False):
    """uint8 [B,H0,W0,3] -> float32 [B*(1+mirror),3,height,width] in [0,1]: the reference's ``transform``
    (scripts/infer.py:25-30) call for call; with ``mirror`` the horizontally flipped copies follow as entries B..2B-1."""
    x = _as_batch(images).to(torch.float32).permute(0, 3, 1, 2).contiguous()
    x = F.interpolate(x, [height, width], mode="bilinear", align_corners=False)
    x /= 255
    return torch.cat([x, x.flip(3)], 0) if mirror else x


def blend_masks(w, dtype=torch.float32, device=None):
    """l_mask, r_mask of batch_post_process_disparity (scripts/eval_depth_pp.py:25-27) over the w columns."""
    l = torch.arange(w, dtype=dtype, device=device) / (w - 1)
    l_mask = 1 - torch.clamp(20 * (l - 0.05), 0, 1)
    return l_mask, l_mask.flip(0)


def postprocess_torch(disp, out_h, out_w, paired=False, a=None, b=None, depth_scale=1.0):
    """Network disparity [B*(1+paired),1,h,w] -> (disp [B,out_h,out_w], depth [B,out_h,out_w]), float32.
    ``paired``: entries B..2B-1 are the predictions of the mirrored images; they are mirrored back and blended with the first
    half (batch_post_process_disparity).  Then the reference's resize (scripts/infer.py:42) and depth_scale / (a disp + b)."""
    if a is None or b is None:
        a, b = disp_to_depth_affine(0.1, 100.0)
    d = disp.to(torch.float32)
    if paired:
        n = d.shape[0] // 2
        l, r = d[:n], d[n:].flip(3)
        l_mask, r_mask = blend_masks(d.shape[3], device=d.device)
        d = r_mask * l + l_mask * r + (1 - l_mask - r_mask) * (0.5 * (l + r))
    d = F.interpolate(d, (out_h, out_w), mode="bilinear", align_corners=False)[:, 0]
    return d, depth_scale / (a * d + b)


def colorize_numpy(x, vmin, vmax, lut=None):
    """float32 [..., n] (or [..., H, W]) with per-image vmin / vmax (scalars or arrays over the leading axis) -> uint8
    [..., 3]: index = clamp(floor((x - vmin) / (vmax - vmin) * 256), 0, 255), every step in float32."""
    lut = magma_lut() if lut is None else lut
    x = np.asarray(x, dtype=np.float32)
    shape = (-1,) + (1,) * (x.ndim - 1)
    lo = np.asarray(vmin, dtype=np.float32).reshape(shape) if np.ndim(vmin) else np.float32(vmin)
    hi = np.asarray(vmax, dtype=np.float32).reshape(shape) if np.ndim(vmax) else np.float32(vmax)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.floor(((x - lo) / (hi - lo)) * np.float32(256))
    idx = np.fmin(np.fmax(t, np.float32(0)), np.float32(255)).astype(np.int64)      # fmax: a NaN (constant image) -> 0
    return lut[idx]


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels

def _device_lut(device):
    key = (device.type, device.index)
    if key not in _lut_device:
        _lut_device[key] = torch.from_numpy(magma_lut().copy()).to(device)
    return _lut_device[key]


def preprocess_hip(images, height, width, mirror=False):
    """preprocess_torch as one launch of td_infer_preprocess; ``images``: uint8 [B,H0,W0,3] on a HIP device."""
    native.ptr(images)          # device and contiguous: the input is never copied
    if images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8:
        raise ValueError("images: uint8 [B,H0,W0,3], got %s %s" % (tuple(images.shape), images.dtype))
    B, H0, W0 = images.shape[:3]
    out = torch.empty(B * (2 if mirror else 1), 3, height, width, device=images.device, dtype=torch.float32)
    native.call("td_infer_preprocess", images, B, H0, W0, height, width, bool(mirror), out)
    return out


def postprocess_hip(disp, out_h, out_w, paired=False, a=None, b=None, depth_scale=1.0, want_depth=True):
    """postprocess_torch as one launch of td_disp_postprocess; ``disp``: fp32 or bf16 [B*(1+paired),1,h,w] on a HIP device."""
    if a is None or b is None:
        a, b = disp_to_depth_affine(0.1, 100.0)
    if disp.dim() != 4 or disp.shape[1] != 1 or disp.dtype not in native.DTYPE_CODES:
        raise ValueError("disp: fp32 / bf16 [N,1,h,w], got %s %s" % (tuple(disp.shape), disp.dtype))
    if paired and disp.shape[0] % 2:
        raise ValueError("paired post-processing needs an even batch, got %d" % disp.shape[0])
    native.require_device(disp)
    disp = disp.contiguous()
    B = disp.shape[0] // (2 if paired else 1)
    h, w = disp.shape[2:]
    d = torch.empty(B, out_h, out_w, device=disp.device, dtype=torch.float32)
    z = torch.empty_like(d) if want_depth else None
    native.call("td_disp_postprocess", disp, disp.dtype, B, h, w, bool(paired), out_h, out_w, a, b, depth_scale, d, z)
    return d, z


def colorize_hip(x, vmin, vmax):
    """colorize_numpy as one launch of td_colorize; x: float32 [B, ...] on a HIP device, vmin / vmax: float32 [B] there."""
    if x.dtype != torch.float32 or x.dim() < 2:
        raise ValueError("x: float32 [B, ...], got %s %s" % (tuple(x.shape), x.dtype))
    x = x.contiguous()
    B = x.shape[0]
    n = x[0].numel()
    vmin = vmin.to(torch.float32).reshape(B).contiguous()
    vmax = vmax.to(torch.float32).reshape(B).contiguous()
    out = torch.empty(tuple(x.shape) + (3,), device=x.device, dtype=torch.uint8)
    native.call("td_colorize", x, B, n, vmin, vmax, _device_lut(x.device), out)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm folding

def _conv_bn_pairs(m):
    """(conv attribute, BatchNorm attribute) of the places a module of this build applies a BatchNorm straight to a
    convolution's output: conv_bn_act / bn_act(bn, conv(x)) in the ResNet stem, BasicBlock, Bottleneck and the
    Sequential(conv, BatchNorm) shortcut.  (The CRP and decoder blocks hold no BatchNorm.)"""
    from mono.model import networks
    if isinstance(m, networks.Bottleneck):
        return [("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3")]
    if isinstance(m, networks.BasicBlock):
        return [("conv1", "bn1"), ("conv2", "bn2")]
    if isinstance(m, networks.ResNet):
        return [("conv1", "bn1")]
    if isinstance(m, nn.Sequential) and len(m) == 2:
        return [("0", "1")]
    return []


def _fold_pair(conv, bn):
    """conv weight / bias with the eval-mode affine of ``bn`` folded in, computed in float32 or higher."""
    dt = torch.promote_types(conv.weight.dtype, torch.float32)
    w = conv.weight.detach().to(dt)
    scale = bn.weight.detach().to(dt) / torch.sqrt(bn.running_var.detach().to(dt) + bn.eps)
    bias = conv.bias.detach().to(dt) if conv.bias is not None else torch.zeros_like(scale)
    bias = (bias - bn.running_mean.detach().to(dt)) * scale + bn.bias.detach().to(dt)
    return (w * scale.view(-1, 1, 1, 1)).to(conv.weight.dtype), bias.to(conv.weight.dtype)


def _own_copy(module):
    """copy.deepcopy(module); activations a forward left on the modules (``features``, ``outputs``: graph tensors, which
    deepcopy refuses) are carried over detached instead."""
    memo = {}
    for m in module.modules():
        for v in vars(m).values():
            items = v.values() if isinstance(v, dict) else v if isinstance(v, (list, tuple)) else (v,)
            for t in items:
                if torch.is_tensor(t) and t.grad_fn is not None:
                    memo[id(t)] = t.detach()
    return copy.deepcopy(module, memo)


def fold_batchnorm(module):
    """A deep copy of ``module`` in eval mode in which every Conv2d followed by this build's BatchNorm carries the
    BatchNorm's eval-mode affine (y = (x - running_mean) / sqrt(running_var + eps) * weight + bias) in its own weight and
    bias, and the BatchNorm is an nn.Identity.  A BatchNorm that is not paired with a convolution stays as it is."""
    from mono.model import networks
    folded = _own_copy(module).eval()
    for m in list(folded.modules()):
        for conv_name, bn_name in _conv_bn_pairs(m):
            conv, bn = getattr(m, conv_name, None), getattr(m, bn_name, None)
            if not (isinstance(conv, nn.Conv2d) and isinstance(bn, networks.BatchNorm) and bn.affine and bn.track_running_stats
                    and bn.num_features == conv.out_channels):
                continue
            w, b = _fold_pair(conv, bn)
            conv.weight = nn.Parameter(w, requires_grad=False)
            conv.bias = nn.Parameter(b, requires_grad=False)
            setattr(m, bn_name, nn.Identity())
    return folded


def count_batchnorms(module):
    return sum(isinstance(m, nn.modules.batchnorm._BatchNorm) for m in module.modules())


# ---------------------------------------------------------------------------------------------------------------------------
# which network runs, and how: shared by DepthPredictor, evaluate.DepthEvaluator, odometry.OdometryEvaluator and cloud.SceneFuser

def check_precision(device, precision, batch_size=None):
    """The constructors' argument check -> torch.device(device): 'fp32' runs on either device, 'bf16' on the HIP device only."""
    if precision not in ("fp32", "bf16"):
        raise ValueError("precision: 'fp32' or 'bf16', got %r" % (precision,))
    if batch_size is not None and int(batch_size) < 1:
        raise ValueError("batch_size: at least 1, got %r" % (batch_size,))
    device = torch.device(device)
    if precision == "bf16" and device.type != "cuda":
        raise ValueError("precision='bf16' is the HIP device's path; the host path is fp32")
    return device


def autocast_for(precision):
    """The context a network call runs under: bf16 autocast for 'bf16' (whose callers hand the network channels-last inputs),
    nothing for 'fp32'."""
    return torch.autocast("cuda", dtype=torch.bfloat16) if precision == "bf16" else contextlib.nullcontext()


@contextlib.contextmanager
def eval_mode(model):
    """``model`` in eval mode; its previous training flag comes back on exit, also when the body raises."""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


def eval_network(model, device, precision):
    """(network to run, context that restores what was changed).  bf16: the BatchNorm-folded copy on ``device``; fp32 with the
    model on another device: its own copy there; fp32 with the model on ``device`` (a model without parameters counts as there,
    and a device without an index matches any): the caller's model itself, inside eval_mode.  The caller's model is never moved."""
    device = torch.device(device)
    if precision == "bf16":
        return fold_batchnorm(model).to(device).eval(), contextlib.nullcontext()
    p = next(model.parameters(), None)
    if p is None or (p.device.type == device.type and (device.index is None or p.device.index == device.index)):
        return model, eval_mode(model)
    return _own_copy(model).to(device).eval(), contextlib.nullcontext()


def network_inputs(x):
    """The evaluation batch of a depth model: no augmentation at inference, so the frame is both ("color", 0, 0) and
    ("color_aug", 0, 0) (the colourisation model reads the former's key even where only the latter is used)."""
    return {("color_aug", 0, 0): x, ("color", 0, 0): x}


class DepthPredictor:
    """predict(images) = postprocess(forward(preprocess(images))).

    model          a depth model of this build (mono_fm, mono_fm_joint*, ...): ``model(network_inputs(x))[("disp", 0, 0)]``.
                   The predictor works on its own copy: the caller's model is never moved, switched to training or changed.
    height, width  the network size (the reference's infer.py hard-codes 320 x 1024; here it is the configuration's)
    device         'cuda[:i]': the three stages run as the kernels of csrc/td_infer.hip; 'cpu': the host statements
    precision      'fp32' (the reference's) or 'bf16': the BatchNorm-folded copy under bf16 autocast, channels-last activations
    post_process   the flip post-processing of scripts/eval_depth_pp.py: the mirrored image goes through the network in the
                   same batch and the two predictions are blended
    depth          depth_scale / (a disp + b); (a, b) = ``affine`` or, by default, those of disp_to_depth(., min_depth, max_depth)
    """

    def __init__(self, model, height, width, device, precision="fp32", post_process=False, min_depth=0.1, max_depth=100.0,
                 depth_scale=1.0, affine=None):
        self.device = check_precision(device, precision)
        self.on_hip = self.device.type == "cuda"
        self.height, self.width = int(height), int(width)
        self.precision = precision
        self.post_process = bool(post_process)
        self.a, self.b = affine if affine is not None else disp_to_depth_affine(min_depth, max_depth)
        self.depth_scale = float(depth_scale)
        own = fold_batchnorm(model) if precision == "bf16" else _own_copy(model)
        self.model = own.to(self.device).eval()
        for p in self.model.parameters():
            p.requires_grad_(False)

    @classmethod
    def from_config(cls, config_path, checkpoint, device=None, **kwargs):
        """Build the configuration's model, load ``checkpoint`` (weights only, strict) and take the network size from
        cfg.data.  The pretrained paths are cleared, as the reference does (scripts/infer.py:50-52)."""
        import tripled_amd  # noqa: F401  (puts mono / mmcv on the path)
        from mmcv import Config
        from mono.model import MONO
        cfg = Config.fromfile(config_path)
        for key in ("depth_pretrained_path", "pose_pretrained_path", "extractor_pretrained_path"):
            cfg.model[key] = None
        model = MONO.module_dict[cfg.model["name"]](cfg.model)
        ckpt = torch.load(checkpoint, map_location="cpu", weights_only=True)      # executes nothing from the file
        model.load_state_dict(ckpt["state_dict"], strict=True)
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        kwargs.setdefault("min_depth", float(cfg.model.get("min_depth", 0.1)))
        kwargs.setdefault("max_depth", float(cfg.model.get("max_depth", 100.0)))
        return cls(model, int(cfg.data["height"]), int(cfg.data["width"]), device, **kwargs)

    # -- stages --------------------------------------------------------------------------------------------------------------
    def preprocess(self, images):
        """same-sized H0 x W0 x 3 uint8 images -> network input [B*(1+post_process),3,height,width] on the device."""
        with torch.no_grad():
            batch = _as_batch(images, self.device)
            if self.on_hip:
                return preprocess_hip(batch, self.height, self.width, self.post_process)
            return preprocess_torch(batch, self.height, self.width, self.post_process)

    def forward(self, x):
        """network input -> network-size disparity [N,1,height,width] (bf16 in the bf16 path)."""
        if self.precision == "bf16":
            x = x.contiguous(memory_format=torch.channels_last)
        with torch.no_grad(), autocast_for(self.precision):
            return self.model(network_inputs(x))[("disp", 0, 0)]

    def postprocess(self, disp_net, out_h, out_w):
        """network-size disparity -> (disp, depth), float32 [B,out_h,out_w]."""
        with torch.no_grad():
            fn = postprocess_hip if self.on_hip else postprocess_torch
            return fn(disp_net, out_h, out_w, self.post_process, self.a, self.b, self.depth_scale)

    def predict(self, images):
        batch = _as_batch(images)
        out_h, out_w = batch.shape[1:3]
        disp_net = self.forward(self.preprocess(batch))
        disp, depth = self.postprocess(disp_net, out_h, out_w)
        return Prediction(disp, depth, disp_net)

    def colorize(self, disp, percentile=95):
        """float32 [B,H,W] (or [H,W]) -> magma picture uint8 [B,H,W,3] ([H,W,3]); vmin = the image's minimum, vmax = its
        ``percentile`` (linear interpolation, np.percentile's default)."""
        with torch.no_grad():
            single = disp.dim() == 2
            d = (disp.unsqueeze(0) if single else disp).to(torch.float32)
            flat = d.reshape(d.shape[0], -1)
            if self.on_hip:
                vmax = torch.stack([torch.quantile(row, percentile / 100.0) for row in flat])
                out = colorize_hip(d.to(self.device), flat.amin(1), vmax)
            else:
                host = flat.cpu().numpy()
                vmax = np.array([np.percentile(row, percentile) for row in host], dtype=np.float32)
                out = torch.from_numpy(colorize_numpy(d.cpu().numpy(), host.min(1), vmax))
            return out[0] if single else out
