"""torch.autograd.Functions over the C ABI of libtripled_hip.so.

These are the fused replacements for the reference's unfused loss ops; each docstring cites
the reference lines it stands in for.  All launches go to torch's current HIP stream and do
not synchronise, so a training step that uses them can be captured in a HIP graph.
"""
import ctypes
import os
import types

import torch

from . import native
from .native import call

_CL = torch.channels_last


def _f32c(t):
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _f32(n, like):
    return torch.empty(n, device=like.device, dtype=torch.float32)


def _cl(t, dtype=None):
    """``t`` in channels-last memory, cast to ``dtype`` if one is given; ``t`` itself when it already is both.  The incoming
    gradient of every node goes through here: the pools, pads and joins keep the gradient's own dtype, the BatchNorm, convolution,
    CRP and bottleneck nodes cast it to the dtype their kernels were launched for."""
    return (t if dtype is None else t.to(dtype)).contiguous(memory_format=_CL)


def _cl_tensor(t, m, dtypes=native.DTYPE_CODES):
    """A 4-D device tensor of one of ``dtypes`` in channels-last memory whose channel count is a multiple of ``m``: what the
    ``*_supported`` predicates below have in common."""
    return t.is_cuda and t.dim() == 4 and t.dtype in dtypes and t.shape[1] % m == 0 and t.is_contiguous(memory_format=_CL)


_BF16 = (torch.bfloat16,)


class PackedFrames:
    """The target and source frames of a step as RGBX pixels ([B,H,W,4] fp32, x = 0), the format the per-scale photometric
    forward reads (csrc/td_common.h "packed frames": one 16-byte load per pixel / bilinear tap instead of three dword loads from
    the NCHW planes), next to the NCHW originals the identity term and the backward read.  The RGBX copies are written by the
    identity-term kernel from the pixels it reads anyway (``photo_identity``), or by td_pack_rgbx when no identity term runs."""

    def __init__(self, tgt, srcs, pack=True):
        self.tgt_planar = _f32c(tgt.detach())
        self.srcs_planar = tuple(_f32c(s.detach()) for s in srcs)
        if self.tgt_planar.dim() != 4 or self.tgt_planar.shape[1] != 3:
            raise ValueError("colour frames are [B,3,H,W], got %s" % (tuple(self.tgt_planar.shape),))
        B, _, H, W = self.tgt_planar.shape
        self.shape = (B, H, W)
        dev = self.tgt_planar.device
        self.tgt = torch.empty(B, H, W, 4, device=dev, dtype=torch.float32)
        self.srcs = tuple(torch.empty(B, H, W, 4, device=dev, dtype=torch.float32) for _ in self.srcs_planar)
        self.packed = False
        if pack:
            self.pack()

    def pack(self):
        if not self.packed:
            B, H, W = self.shape
            for planar, out in zip((self.tgt_planar,) + self.srcs_planar, (self.tgt,) + self.srcs):
                call("td_pack_rgbx", planar, B, H, W, out)
            self.packed = True
        return self


def pack_frames(tgt, srcs, pack=True):
    """``pack=False``: the RGBX copies are left to ``photo_identity`` (which writes them as a by-product)."""
    return PackedFrames(tgt, srcs, pack)


def _frames(tgt, srcs):
    return tgt.pack() if isinstance(tgt, PackedFrames) else PackedFrames(tgt, srcs)


def photo_identity(tgt, srcs=None):
    """Auto-mask identity term for every source frame, once per step.
    compute_reprojection_loss(inputs[("color", f, 0)], target) at
    mono/model/mono_fm_joint_inpaint/net.py:101-104 -> [B, n_src, H, W] (a view: the memory is [B,H,W,n_src], the layout
    td_photo_fwd reads).  ``tgt``: the [B,3,H,W] target with ``srcs`` the list of sources, or a PackedFrames -- whose RGBX copies
    this call fills if they are not packed yet."""
    fr = tgt if isinstance(tgt, PackedFrames) else PackedFrames(tgt, srcs, pack=False)
    B, H, W = fr.shape
    out = torch.empty(B, H, W, len(fr.srcs), device=fr.tgt.device, dtype=torch.float32)
    emit = not fr.packed
    call("td_photo_identity", fr.tgt_planar, fr.srcs_planar, len(fr.srcs), B, H, W, out, fr.tgt if emit else None,
         fr.srcs if emit else None)
    fr.packed = True
    return out.permute(0, 3, 1, 2)


def area_downsample(img, h, w):
    """F.interpolate(img, (h, w), mode='area') for integer factors
    (mono/model/mono_fm_joint/net.py:283, :311).  No gradient (the image is an input)."""
    img = _f32c(img.detach())
    B, C, H, W = img.shape
    if (H, W) == (h, w):
        return img
    out = torch.empty(B, C, h, w, device=img.device, dtype=torch.float32)
    call("td_area_downsample", img, B, C, H, W, h, w, out)
    return out


class _PhotometricScaleLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, P, tgt, srcs, tgt_planar, srcs_planar, invK, idloss, noise, min_depth, max_depth, n_scales, keep_warped):
        disp = _f32c(disp)
        P = _f32c(P)
        B, H, W, _ = tgt.shape                     # RGBX frames [B,H,W,4]
        hs, ws = disp.shape[2], disp.shape[3]
        n_src = len(srcs)
        dev = tgt.device
        argmin = torch.empty(B, H, W, device=dev, dtype=torch.uint8)
        nblk = native.load().td_photo_num_blocks(B, H, W)
        partial = torch.empty(nblk, device=dev, dtype=torch.float32)
        warped = torch.empty(n_src, B, 3, H, W, device=dev, dtype=torch.float32) if keep_warped else None
        loss = torch.empty(1, device=dev, dtype=torch.float32)
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        coef = torch.empty(B, 9, H, W, device=dev, dtype=torch.float32) if need_grad else None
        call("td_photo_fwd", tgt, srcs, n_src, disp, P, invK, idloss, noise, B, H, W, hs, ws, float(min_depth), float(max_depth),
             argmin, warped, None, partial, coef)
        inv_count = 1.0 / (float(B) * H * W * n_scales)
        call("td_sum_scaled", partial, nblk, inv_count, loss)
        ctx.save_for_backward(disp, P, tgt_planar, invK, argmin, coef if coef is not None else argmin, tgt, *srcs_planar, *srcs)
        ctx.meta = (min_depth, max_depth, inv_count, idloss is not None, n_src)
        ctx.mark_non_differentiable(argmin)
        if keep_warped:
            ctx.mark_non_differentiable(warped)
            return loss.reshape(()), argmin, warped
        return loss.reshape(()), argmin, torch.empty(0, device=dev)

    @staticmethod
    def backward(ctx, g_loss, _g_argmin, _g_warped):
        disp, P, tgt, invK, argmin, coef, tgt_x, *both = ctx.saved_tensors
        min_depth, max_depth, inv_count, automask, n_src = ctx.meta
        srcs, srcs_x = both[:n_src], both[n_src:]      # NCHW frames, and their RGBX copies (read at the finest scale)
        B, _, H, W = tgt.shape                     # NCHW frames
        hs, ws = disp.shape[2], disp.shape[3]
        dev = tgt.device
        g = _f32c(g_loss.reshape(1))
        d_up = torch.empty(n_src, B, H, W, device=dev, dtype=torch.float32)      # one plane per source frame
        nblk = native.load().td_photo_bwd_num_blocks(B, H, W)
        dP_part = torch.empty(nblk, n_src * 12, device=dev, dtype=torch.float32)
        call("td_photo_bwd", tgt, srcs, tgt_x, srcs_x, n_src, disp, P, invK, argmin, coef, automask, g, inv_count, B, H, W, hs, ws,
             float(min_depth), float(max_depth), d_up, dP_part)
        d_disp = torch.empty_like(disp)
        call("td_upsample_adjoint_planes", d_up, n_src, B, H, W, hs, ws, d_disp, 0)
        dP = torch.empty_like(P)
        call("td_reduce_dP", dP_part, n_src, B, H, W, dP)
        return d_disp, dP, None, None, None, None, None, None, None, None, None, None, None


def photometric_scale_loss(disp, P, tgt, srcs, invK, idloss=None, noise=None, min_depth=0.1,
                           max_depth=100.0, n_scales=4, keep_warped=False):
    """One scale of generate_images_pred + automask + min-reprojection
    (mono/model/mono_fm_joint/net.py:181-194; mono/model/mono_fm_joint_inpaint/net.py:101-117).

    disp [B,1,hs,ws]; P [n_src,B,3,4] = (K @ T)[:, :3, :] per source frame; ``tgt`` [B,3,H,W] with ``srcs``, or a PackedFrames
    (``srcs`` ignored); idloss [B,n_src,H,W] from photo_identity (None = no automask); noise [n_src,B,H,W] N(0,1) draws or None.
    Returns (loss = mean(min)/n_scales, argmin uint8 [B,H,W], warped [n_src,B,3,H,W] or empty).
    """
    fr = _frames(tgt, srcs)                        # RGBX frames (packed here unless the caller packed them once per step)
    invK = _f32c(invK)
    if idloss is not None:
        # the kernel reads [B,H,W,n_src]; photo_identity's result is a [B,n_src,H,W] VIEW of exactly that memory
        idloss = idloss.permute(0, 2, 3, 1)
        if idloss.dtype != torch.float32 or not idloss.is_contiguous():
            idloss = idloss.float().contiguous()
    if noise is not None:
        noise = _f32c(noise)
    return _PhotometricScaleLoss.apply(disp, P, fr.tgt, fr.srcs, fr.tgt_planar, fr.srcs_planar, invK, idloss, noise, min_depth,
                                       max_depth, n_scales, keep_warped)


class _SmoothLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, img, normalize, weight):
        disp = _f32c(disp)
        B, _, h, w = disp.shape
        mean = _f32(B, disp)
        nblk = native.load().td_smooth_num_blocks(B, h, w)
        partial = torch.empty(nblk, 6, device=disp.device, dtype=torch.float32)
        loss = _f32(1, disp)
        call("td_smooth_fwd", disp, img, B, h, w, int(normalize), mean, partial)
        call("td_smooth_finish", partial, B, h, w, float(weight), loss)
        ctx.save_for_backward(disp, img, mean)
        ctx.meta = (bool(normalize), float(weight), nblk)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        disp, img, mean = ctx.saved_tensors
        normalize, weight, nblk = ctx.meta
        B, _, h, w = disp.shape
        g = _f32c(g_loss.reshape(1))
        g_hat = torch.empty(B, h, w, device=disp.device, dtype=torch.float32)
        dot = _f32(nblk, disp)
        d_disp = torch.empty_like(disp)
        call("td_smooth_bwd", disp, img, mean, B, h, w, normalize, g, weight, g_hat, dot, d_disp, 0)
        return d_disp, None, None, None


def smooth_loss(disp, img_at_scale, normalize=True, weight=1.0):
    """weight * get_smooth_loss(disp / (mean(disp) + 1e-7), img)
    (mono/model/mono_fm_joint_inpaint/net.py:122-131, mono/model/mono_fm_joint/net.py:279-307).
    ``img_at_scale`` is the target area-resized to disp's size (area_downsample)."""
    img = _f32c(img_at_scale)
    if img.shape[2:] != disp.shape[2:]:
        raise ValueError("img_at_scale must already have disp's spatial size")
    return _SmoothLoss.apply(disp, img, normalize, weight)


def _raw(t):
    """Device pointer of ``t`` with NO check: for the two ops that take a tensor of any dense layout (robust_l1_map,
    quantize_fp8 -- their wrappers check density themselves); everything else hands native.call the tensor."""
    return ctypes.c_void_p(t.data_ptr())


def _empty_cl(n, c, h, w, like, dtype=None):
    return torch.empty((n, c, h, w), device=like.device, dtype=dtype or like.dtype, memory_format=_CL)


def _pool_fwd(name, ctx, x, stride):
    N, C, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = _empty_cl(N, C, Ho, Wo, x)
    idx = torch.empty((N, Ho, Wo, C), device=x.device, dtype=torch.uint8)
    call(name, x, x.dtype, N, H, W, C, out, idx)
    ctx.save_for_backward(idx)
    ctx.in_hw = (H, W)
    return out


def _pool_bwd(name, ctx, g):
    (idx,) = ctx.saved_tensors
    N, _, _, C = idx.shape
    H, W = ctx.in_hw
    g = _cl(g)
    gin = _empty_cl(N, C, H, W, g)
    call(name, g, idx, g.dtype, N, H, W, C, gin)
    return gin


class _MaxPool5(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _pool_fwd("td_maxpool5_fwd", ctx, x, 1)

    @staticmethod
    def backward(ctx, g):
        return _pool_bwd("td_maxpool5_bwd", ctx, g)


class _MaxPool3s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _pool_fwd("td_maxpool3s2_fwd", ctx, x, 2)

    @staticmethod
    def backward(ctx, g):
        return _pool_bwd("td_maxpool3s2_bwd", ctx, g)


def maxpool3s2(x):
    """nn.MaxPool2d(3, 2, 1) on a channels_last CUDA tensor (reference: resnet.py:101)."""
    if not maxpool5_supported(x):
        raise native.NativeLibraryError("maxpool3s2 needs a channels_last f32/bf16 HIP tensor with C % 8 == 0")
    return _MaxPool3s2.apply(x)


def maxpool5_supported(x):
    return _cl_tensor(x, 8)


def maxpool5(x):
    """nn.MaxPool2d(5, 1, 2) on a channels_last CUDA tensor (reference: layers.py:208,213)."""
    if not maxpool5_supported(x):
        raise native.NativeLibraryError("maxpool5 needs a channels_last f32/bf16 HIP tensor with C % 8 == 0")
    return _MaxPool5.apply(x)


class _CRP(torch.autograd.Function):
    """Chained residual pooling (reference: CRPBlock, mono/model/mono_fm_joint/layers.py:200-215): top_0 = x,
    top_i = conv1x1_i(maxpool5(top_{i-1})), out = x + sum_i top_i -- as ONE autograd node over hand-written kernels:

      forward   per stage: the 5x5 pool (column march) and the pointwise convolution on the MFMA GEMM whose epilogue also
                advances the running sum (td_conv1x1_fwd_sum: two outputs, no separate add pass)
      backward  per stage, last to first: weight gradient (td_conv1x1_wgrad), data gradient (td_conv1x1_dgrad) and the pool's
                backward with the gradient the stage's input ALSO receives straight from the running sum added while it is
                written out (td_maxpool5_bwd_add): autograd's gradient-accumulation adds are gone

    Against the per-op nodes: 8 tensor adds per block and direction fewer, and the twelve 1x1 convolution calls of a block
    (forward / data / weight gradient through MIOpen / CK, the weight gradients with their zero-fill and cast passes) run on the
    deterministic hand-written GEMMs."""

    @staticmethod
    def forward(ctx, x, *ws):
        Nb, C, H, W = x.shape
        M = Nb * H * W
        top, run = x, x
        saved = []
        for w in ws:
            pooled = torch.empty_like(x, memory_format=_CL)
            idx = torch.empty((Nb, H, W, C), device=x.device, dtype=torch.uint8)
            call("td_maxpool5_fwd", top, x.dtype, Nb, H, W, C, pooled, idx)
            top = torch.empty_like(x, memory_format=_CL)
            run_out = torch.empty_like(x, memory_format=_CL)
            call("td_conv1x1_fwd_sum", pooled, w, M, C, C, run, top, run_out)
            run = run_out
            saved += [pooled, idx]
        ctx.save_for_backward(*ws, *saved)
        ctx.n = len(ws)
        return run

    @staticmethod
    def backward(ctx, g):
        with wgrad_group():      # the node's 1x1 weight gradients leave as one grouped launch at the end
            return _CRP._backward(ctx, g)

    @staticmethod
    def _backward(ctx, g):
        n = ctx.n
        ws, saved = ctx.saved_tensors[:n], ctx.saved_tensors[n:]
        Nb, C, H, W = g.shape
        M = Nb * H * W
        g = _cl(g, torch.bfloat16)
        g_top = g
        dws = [None] * n
        for i in reversed(range(n)):
            w, pooled, idx = ws[i], saved[2 * i], saved[2 * i + 1]
            dws[i] = conv1x1_wgrad(g_top, pooled, w, M, C, C, H, W, 1)
            d_pool = torch.empty_like(g, memory_format=_CL)
            call("td_conv1x1_dgrad", g_top, w, M, 1, C, C, None, d_pool)
            g_prev = torch.empty_like(g, memory_format=_CL)
            call("td_maxpool5_bwd_add", d_pool, idx, g, g.dtype, Nb, H, W, C, g_prev)
            g_top = g_prev
        return (g_top,) + tuple(dws)


def _weight_1x1_ok(w):
    return w.dtype == torch.bfloat16 and (w.is_contiguous() or w.is_contiguous(memory_format=_CL))


def crp_supported(x, ws):
    C = x.shape[1]
    return (_cl_tensor(x, 64, _BF16) and len(ws) >= 1
            and all(_weight_1x1_ok(w) and tuple(w.shape) == (C, C, 1, 1) for w in ws))


def crp_block(x, ws):
    """x + sum_i top_i, top_i = conv1x1(maxpool5(top_{i-1}), ws[i]) (reference: layers.py:200-215) on bf16 channels_last HIP
    tensors with C % 64 == 0 (one autograd node, see _CRP)."""
    if not crp_supported(x, ws):
        raise native.NativeLibraryError("crp_block needs a bf16 channels_last HIP tensor with C % 64 == 0 and [C, C, 1, 1] weights")
    return _CRP.apply(x, *ws)


class _JoinChannels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, tail):
        N, C0, H, W = a.shape
        C1, C2 = b.shape[1], tail.shape[1]
        out = _empty_cl(N, C0 + C1 + 8, H, W, a)
        call("td_join_fwd", a, b, tail, a.dtype, N * H * W, C0, C1, C2, out)
        ctx.dims = (N, C0, C1, C2, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        N, C0, C1, C2, H, W = ctx.dims
        g = _cl(g)
        ga, gb, gt = _empty_cl(N, C0, H, W, g), _empty_cl(N, C1, H, W, g), _empty_cl(N, C2, H, W, g)
        call("td_join_bwd", g, g.dtype, N * H * W, C0, C1, C2, ga, gb, gt)
        return ga, gb, gt


class _JoinChannelsUp2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b_half, tail):
        N, C0, H, W = a.shape
        C1, C2 = b_half.shape[1], tail.shape[1]
        out = _empty_cl(N, C0 + C1 + 8, H, W, a)
        call("td_join_up2_fwd", a, b_half, tail, a.dtype, N, H, W, C0, C1, C2, out)
        ctx.dims = (N, C0, C1, C2, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        N, C0, C1, C2, H, W = ctx.dims
        g = _cl(g)
        ga, gb, gt = _empty_cl(N, C0, H, W, g), _empty_cl(N, C1, H // 2, W // 2, g), _empty_cl(N, C2, H, W, g)
        call("td_join_up2_bwd", g, g.dtype, N, H, W, C0, C1, C2, ga, gb, gt)
        return ga, gb, gt


def _join_operands_ok(a, b, tail):
    """What both joins ask of their operands, but for b's spatial size: a and b with C % 8 == 0, a tail of 1..8 channels over
    a's pixels, one dtype, one batch."""
    return (_cl_tensor(a, 8) and _cl_tensor(b, 8) and _cl_tensor(tail, 1) and b.dtype == a.dtype and tail.dtype == a.dtype
            and 1 <= tail.shape[1] <= 8 and a.shape[0] == b.shape[0] == tail.shape[0] and a.shape[2:] == tail.shape[2:])


def join_channels_up2_supported(a, b_half, tail):
    return (_join_operands_ok(a, b_half, tail)
            and a.shape[2] == 2 * b_half.shape[2] and a.shape[3] == 2 * b_half.shape[3])


def join_channels_up2(a, b_half, tail):
    """torch.cat((a, upsample_x2_nearest(b_half), tail, zeros), 1) up to C0 + C1 + 8 channels, without materialising the
    up-sampled operand (reference: depth_decoder.py:89-103, where x was up-sampled at the end of the previous stage)."""
    if not join_channels_up2_supported(a, b_half, tail):
        raise native.NativeLibraryError("join_channels_up2 needs channels_last f32/bf16 HIP tensors, b at half resolution")
    return _JoinChannelsUp2.apply(a, b_half, tail)


def join_channels_supported(a, b, tail):
    return _join_operands_ok(a, b, tail) and a.shape[2:] == b.shape[2:]


def join_channels(a, b, tail):
    """torch.cat((a, b, tail, zeros), 1) up to C0 + C1 + 8 channels on channels_last HIP tensors
    (reference: depth_decoder.py:89-103 plus the channel-alignment padding of Conv3x3)."""
    if not join_channels_supported(a, b, tail):
        raise native.NativeLibraryError("join_channels needs channels_last f32/bf16 HIP tensors, C0 % 8 == C1 % 8 == 0, C2 <= 8")
    return _JoinChannels.apply(a, b, tail)


# ---- BatchNorm plumbing shared by _BatchNormAct, _Conv1x1BatchNormAct, _Bottleneck and _SyncBatchNormAct ------------------
def _conv1x1_stats(x, w, groups, stride):
    """The 1x1 convolution on the MFMA GEMM with the BatchNorm statistics of its output taken in the epilogue:
    (z bf16, partials, their rows per group)."""
    Nb, K, Hi, Wi = x.shape
    N = w.shape[0]
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    M = Nb * Ho * Wo
    z = _empty_cl(Nb, N, Ho, Wo, x, torch.bfloat16)
    S = native.load().td_conv1x1_stat_rows(M, groups, N)
    part = _f32(groups * S * N * 2, x)
    call("td_conv1x1_fwd", x, w, M, groups, K, N, Hi, Wi, stride, z, part)
    return z, part, S


class BnState:
    """What a BatchNorm layer contributes to a fused block: affine parameters are passed as tensors (autograd), the rest here."""
    __slots__ = ("running_mean", "running_var", "momentum", "eps")

    def __init__(self, bn):
        self.running_mean, self.running_var = bn.running_mean, bn.running_var
        self.momentum, self.eps = float(bn.momentum), float(bn.eps)


def _bn_apply(z, part, S, gamma, beta, st, residual, relu, groups):
    """relu?(batch_norm(z) [+ residual]) with the statistics finished from ``part`` in the kernel's prologue:
    (y, mean, invstd); ``st``: the layer's BnState, or its four fields under those names."""
    Nb, C, H, W = z.shape
    y = torch.empty_like(z, memory_format=_CL)
    mean, invstd = _f32(groups * C, z), _f32(groups * C, z)
    call("td_bn_fwd_from_partials", z, residual, z.dtype, gamma, beta, st.running_mean, st.running_var, st.momentum, st.eps,
         int(relu), Nb * H * W, groups, C, part, S, y, mean, invstd)
    return y, mean, invstd


def _dres(x, dy, has_res, relu):
    """The residual's gradient as (the buffer the backward kernel writes, what the node returns).  relu + residual: the masked
    gradient is a second output of the kernel; residual without relu: it is dy itself and the kernel gets no buffer."""
    if not has_res:
        return None, None
    if relu:
        buf = torch.empty_like(x, memory_format=_CL)
        return buf, buf
    return None, dy


def _bn_backward(dy, x, y, gamma, beta, mean, invstd, relu, has_res, groups):
    """td_bn_bwd of relu?(batch_norm(x) [+ residual]); ``y`` is the saved output where the ReLU mask cannot be re-derived from
    x (relu + residual), else None.  -> (dx, dres, dgamma f32, dbeta f32), in x's dtype."""
    Nb, C, H, W = x.shape
    M = Nb * H * W
    dx = torch.empty_like(x, memory_format=_CL)
    buf, dres = _dres(x, dy, has_res, relu)
    dgamma, dbeta = _f32(C, x), _f32(C, x)
    ws = _f32(native.load().td_bn_workspace_floats(M, groups, C), x)
    call("td_bn_bwd", dy, x, y, x.dtype, gamma, beta, mean, invstd, int(relu), M, groups, C, dx, buf, dgamma, dbeta, ws)
    return dx, dres, dgamma, dbeta


def _residual(residual, x):
    """The residual operand in x's dtype and channels-last memory (itself when it already is; None stays None)."""
    return None if residual is None else _cl(residual, x.dtype)


class _BatchNormAct(torch.autograd.Function):
    """F.batch_norm(training=True) [+ residual] [-> relu] on a channels_last tensor, three launches each way."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, residual, momentum, eps, relu, groups):
        N, C, H, W = x.shape
        M = N * H * W
        y = torch.empty_like(x, memory_format=_CL)
        mean, invstd = _f32(groups * C, x), _f32(groups * C, x)
        ws = _f32(native.load().td_bn_workspace_floats(M, groups, C), x)
        call("td_bn_fwd", x, residual, x.dtype, weight, bias, running_mean, running_var, float(momentum), float(eps), int(relu),
             M, groups, C, y, mean, invstd, ws)
        # the ReLU mask is re-derived from x in backward unless a residual went into the pre-activation
        ctx.save_for_backward(x, y if (relu and residual is not None) else None, weight, bias, mean, invstd)
        ctx.relu, ctx.has_res, ctx.groups = bool(relu), residual is not None, groups
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, weight, bias, mean, invstd = ctx.saved_tensors
        dx, dres, dgamma, dbeta = _bn_backward(_cl(dy, x.dtype), x, y, weight, bias, mean, invstd, ctx.relu, ctx.has_res, ctx.groups)
        return dx, dgamma.to(weight.dtype), dbeta.to(weight.dtype), None, None, dres, None, None, None, None


class _Conv1x1BatchNormAct(torch.autograd.Function):
    """relu?( batch_norm( conv1x1(x, w) ) [+ residual] ) with the convolution on the hand-written MFMA GEMM and the batch
    statistics taken from its epilogue (no statistics pass over the convolution output): GEMM, [shrink of the partial rows when
    there are more than 96], apply with the statistics finished in its prologue.  Backward: td_bn_bwd, the data gradient through
    ATen (MIOpen), the weight gradient on the hand-written MFMA kernel (td_conv1x1_wgrad).  (The bottlenecks of the training
    step take the block-level node _Bottleneck since round 4; this per-layer node serves the BasicBlock down-sample branch and
    TD_NO_FUSED_BLOCK.)"""

    @staticmethod
    def forward(ctx, x, w, weight, bias, running_mean, running_var, residual, momentum, eps, relu, groups, stride):
        yc, part, S = _conv1x1_stats(x, w, groups, stride)
        st = types.SimpleNamespace(running_mean=running_mean, running_var=running_var, momentum=float(momentum), eps=float(eps))
        y, mean, invstd = _bn_apply(yc, part, S, weight, bias, st, residual, relu, groups)
        ctx.save_for_backward(x, w, yc, y if (relu and residual is not None) else None, weight, bias, mean, invstd)
        ctx.relu, ctx.has_res, ctx.groups, ctx.stride = bool(relu), residual is not None, groups, stride
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, yc, y, weight, bias, mean, invstd = ctx.saved_tensors
        Nb, N, Ho, Wo = yc.shape
        dyc, dres, dgamma, dbeta = _bn_backward(_cl(dy, yc.dtype), yc, y, weight, bias, mean, invstd, ctx.relu, ctx.has_res,
                                                ctx.groups)
        dx = dw = None
        if ctx.needs_input_grad[0]:      # data gradient: MIOpen / CK
            dx = torch.ops.aten.convolution_backward(dyc, x, w, None, [ctx.stride, ctx.stride], [0, 0], [1, 1], False, [0, 0], 1,
                                                     [True, False, False])[0]
        if ctx.needs_input_grad[1]:      # weight gradient: hand-written MFMA kernel (transposed LDS reads, ordered slab sum)
            K, Hi, Wi = x.shape[1], x.shape[2], x.shape[3]
            dw = conv1x1_wgrad(dyc, x, w, Nb * Ho * Wo, K, N, Hi, Wi, ctx.stride)
        return dx, dw, dgamma.to(weight.dtype), dbeta.to(weight.dtype), None, None, dres, None, None, None, None, None


def conv1x1_bn_act_supported(x, w, bn_weight, stride=1):
    return (_cl_tensor(x, 64, _BF16) and w.dim() == 4 and _weight_1x1_ok(w)
            and w.shape[2] == 1 and w.shape[3] == 1 and w.shape[1] == x.shape[1] and w.shape[0] % 64 == 0
            and stride in (1, 2) and bn_weight is not None and bn_weight.dtype == torch.float32)


def conv1x1_bn_act(x, w, weight, bias, running_mean, running_var, momentum, eps, residual=None, relu=False, groups=1, stride=1):
    """conv1x1 -> training-mode BatchNorm2d -> [+ residual] -> [relu] (reference: resnet.py:66-86 conv1/bn1, conv3/bn3 and the
    down-sample branch :119-127) for bf16 channels_last HIP tensors, Cin % 64 == Cout % 64 == 0."""
    if x.shape[0] % groups:
        raise ValueError("batch %d is not %d stacked passes" % (x.shape[0], groups))
    if not conv1x1_bn_act_supported(x, w, weight, stride):
        raise native.NativeLibraryError("conv1x1_bn_act needs bf16 channels_last HIP tensors with Cin % 64 == Cout % 64 == 0")
    return _Conv1x1BatchNormAct.apply(x, w, weight, bias, running_mean, running_var, _residual(residual, x), momentum, eps, relu,
                                      groups, stride)


ACT_CODES = {None: 0, "elu": 1, "leaky_relu": 2}


class _ConvBiasAct(torch.autograd.Function):
    """act(conv2d(x, w) + b) for a stride-1 unpadded convolution (the decoders' Conv3x3 after its reflection pad): the
    convolution through MIOpen WITHOUT its bias, then bias + activation in one in-place pass (td_bias_act_fwd); backward: the
    activation's adjoint and the bias gradient in one pass (td_bias_act_bwd) in front of MIOpen's data / weight gradients.
    Reference: ConvBlock (layers.py:143-155), depth_decoder.py:89-103."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        y = _cl(torch.ops.aten.convolution(x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1))
        B, C, H, W = y.shape
        call("td_bias_act_fwd", y, b, b.dtype if b is not None else 0, y.dtype, B * H * W, C, ACT_CODES[act], y)
        ctx.save_for_backward(x, w, y if act is not None else None, b)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, a, b = ctx.saved_tensors
        B, C, H, W = g.shape
        g = _cl(g, w.dtype)
        M = B * H * W
        gy = torch.empty_like(g, memory_format=_CL) if ctx.act is not None else g
        db = torch.empty_like(b) if b is not None and ctx.needs_input_grad[2] else None
        ws = _f32(native.load().td_bias_act_workspace_floats(M, C), g)
        if ctx.act is not None or db is not None:
            call("td_bias_act_bwd", g, a, g.dtype, M, C, ACT_CODES[ctx.act], gy if ctx.act is not None else None, db,
                 db.dtype if db is not None else 0, ws)
        dx, dw, _ = torch.ops.aten.convolution_backward(gy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                        [ctx.needs_input_grad[0], ctx.needs_input_grad[1], False])
        return dx, dw, db, None


def conv_bias_act_supported(x, w, b, act):
    cout = w.shape[0]
    return (act in ACT_CODES and _cl_tensor(x, 1, _BF16) and w.dtype == torch.bfloat16
            and (b is None or b.dtype in native.DTYPE_CODES)
            and 8 <= cout <= 256 and cout % 8 == 0 and 256 % (cout // 8) == 0 and x.shape[1] == w.shape[1])


def conv_bias_act(x, w, b, act=None):
    """act(F.conv2d(x, w, b)) (stride 1, no padding) with bias + activation and their adjoints fused (see _ConvBiasAct)."""
    if not conv_bias_act_supported(x, w, b, act):
        raise native.NativeLibraryError("conv_bias_act needs bf16 channels_last HIP tensors, Cout in {8, 16, 32, 64, 128, 256}")
    return _ConvBiasAct.apply(x, w, b, act)


# ---- weight gradients of the 1x1 convolutions: immediate, or enqueued and launched as one group ---------------------------
_WGRAD_QUEUE = None          # the innermost active wgrad_group, or None
WGRAD_GROUP = os.environ.get("TD_WGRAD_GROUP", "node")      # "node" | "step" | "off"


class wgrad_group:
    """A scope whose 1x1 weight gradients (conv1x1_wgrad) are ENQUEUED and launched together at its exit by
    td_conv1x1_wgrad_group -- 2 launches per <= 40 problems instead of 2 per problem, bit-equal results.

    ``assign=False`` (a backward node around its own three or four weight gradients: scope "node"): conv1x1_wgrad returns the
    output tensor at once and the exit, still inside the node's backward, writes it -- autograd never sees an unwritten buffer.
    ``assign=True`` (around a whole ``loss.backward()``: scope "step", TD_WGRAD_GROUP=step): a deferred node hands autograd NO
    gradient for its weight (None); the exit computes the group and then stores (first use) or adds (a weight used twice) each
    result into ``weight.grad`` itself.  Only leaf weights are deferred that way and per-parameter gradient hooks do not see
    them, so tripled_amd.step.TrainStep allows it only with the flat parameter store and without the overlapped bucket engine.
    Measured (profiles/r04/wgrad_group_v1.txt): "step" is SLOWER than no grouping -- at the end of backward every dz and x comes
    from HBM again, while the immediate launches find them in L2 / MALL -- so "node" is the default."""

    def __init__(self, assign=False, scope="node"):
        self.assign, self.scope, self.items = assign, scope, []

    def __enter__(self):
        global _WGRAD_QUEUE
        self.prev = _WGRAD_QUEUE
        # an inner "node" scope inside an active "step" scope leaves the queue of the step in place
        self.active = WGRAD_GROUP == self.scope and not (self.prev is not None and self.prev.assign)
        if self.active:
            _WGRAD_QUEUE = self
        return self

    def __exit__(self, *exc):
        global _WGRAD_QUEUE
        if self.active:
            _WGRAD_QUEUE = self.prev
            if self.items and exc[0] is None:
                flush_wgrads(self.items)
        return False


def deferred_wgrads():
    """``with deferred_wgrads(): loss.backward()`` -- the "step" scope of wgrad_group (active under TD_WGRAD_GROUP=step)."""
    return wgrad_group(assign=True, scope="step")


def flush_wgrads(queue):
    ints = lambda key: native.int_array([q[key] for q in queue])
    tensors = lambda key: [q[key] for q in queue]      # (the queue keeps them alive until the launch is enqueued)
    call("td_conv1x1_wgrad_group", len(queue), tensors("dy"), tensors("x"), (ctypes.c_longlong * len(queue))(*[q["M"] for q in queue]),
         ints("K"), ints("N"), ints("Hi"), ints("Wi"), ints("stride"),
         native.int_array([native.DTYPE_CODES[q["dw"].dtype] for q in queue]), tensors("dw"), tensors("ws"))
    for q in queue:
        w = q["w"]
        if w is None:
            continue
        if w.grad is None:
            w.grad = q["dw"]
        else:
            w.grad.add_(q["dw"])


def conv1x1_wgrad(dz, inp, w, M, K, N, Hi, Wi, stride):
    """dW of a 1x1 convolution (td_conv1x1_wgrad) for an autograd backward to return: launched now, or enqueued in the
    innermost wgrad_group -- which returns the tensor its exit will write ("node" scope), or None for a leaf weight whose
    .grad the exit fills in ("step" scope)."""
    dw = torch.empty_like(w)
    wsw = _f32(native.load().td_conv1x1_wgrad_workspace_floats(M, K, N), dz)
    q = _WGRAD_QUEUE
    if q is not None and (not q.assign or (w.is_leaf and w.requires_grad)):
        q.items.append(dict(dy=dz, x=inp, dw=dw, ws=wsw, w=w if q.assign else None, M=M, K=K, N=N, Hi=Hi, Wi=Wi, stride=stride))
        return None if q.assign else dw
    call("td_conv1x1_wgrad", dz, inp, M, K, N, Hi, Wi, stride, w.dtype, dw, wsw)
    return dw


def conv3x3_wgrad_wins(B, Ho, Wo, C, N, stride):
    """Dispatch table of td_conv3x3_wgrad, from profiles/r04/conv3x3_wgrad_bench_v2.txt: the kernel beats MIOpen's weight
    gradient (its zero-fill and cast passes included) on the 64-channel maps of 48 x 160 and larger; everywhere else MIOpen is
    20-45 % faster and keeps the layer."""
    return stride == 1 and C == 64 and N == 64 and Wo >= 160 and Ho >= 48 and B * Ho * Wo < (1 << 31) - 128


def conv3x3_wgrad(dy, x, w, pad):
    """dW of a 3x3 stride-1 convolution (td_conv3x3_wgrad): dy [B,N,Ho,Wo], x [B,C,Hi,Wi] bf16 channels_last -> like w."""
    B, N, Ho, Wo = dy.shape
    C = x.shape[1]
    dw = torch.empty_like(w, memory_format=_CL)
    ws = _f32(native.load().td_conv3x3_wgrad_workspace_floats(B, Ho, Wo, C, N), x)
    call("td_conv3x3_wgrad", dy, x, B, Ho, Wo, C, N, pad, w.dtype, dw, ws)
    return dw


class _Bottleneck(torch.autograd.Function):
    """The whole ResNet bottleneck (reference: Bottleneck.forward, mono/model/mono_fm_joint/resnet.py:66-86) as ONE autograd
    node, so that BatchNorm work can ride on the neighbouring 1x1 GEMMs across layer boundaries (csrc/td_conv1x1.hip, "fused
    forms"):

      forward   conv1 GEMM (+ bn1 statistics) -> bn1 apply + relu -> conv2 (3x3: MIOpen) -> bn2 statistics pass
                -> conv3 GEMM with relu(bn2(.)) applied to its operand while it is staged (+ bn3 statistics)
                -> [down-sample GEMM + bn] -> bn3 apply + identity + relu
      backward  bn3 backward -> conv3 data gradient whose epilogue forms bn2's backward sums; conv3 weight gradient
                -> bn2 dx -> conv2 backward (MIOpen) -> bn1 statistics pass
                -> conv1 data gradient with bn1's backward applied to its operand while it is staged and the identity
                   branch's gradient added in its epilogue; conv1 weight gradient

    Against the per-layer nodes this drops the bn2 apply pass, the bn2 backward statistics pass, the bn1 dx pass and the
    residual-gradient add (4 launches and their passes over the activations per block), and both data gradients run on the
    hand-written MFMA GEMM."""

    @staticmethod
    def forward(ctx, x, w1, w2, w3, g1, b1, g2, b2, g3, b3, wd, gd, bd, st1, st2, st3, std, groups, stride):
        lib = native.load()
        Nb = x.shape[0]
        c, Cout = w1.shape[0], w3.shape[0]

        # conv1 -> bn1 -> relu
        z1, p1, S1 = _conv1x1_stats(x, w1, groups, 1)
        a1, mean1, invstd1 = _bn_apply(z1, p1, S1, g1, b1, st1, None, True, groups)
        # conv2 (3x3, stride s): MIOpen
        z2 = _cl(torch.ops.aten.convolution(a1, w2, None, [stride, stride], [1, 1], [1, 1], False, [0, 0], 1))
        Ho, Wo = z2.shape[2], z2.shape[3]
        M2 = Nb * Ho * Wo
        # bn2 statistics pass; its apply + relu ride on conv3's operand staging
        R2 = lib.td_bn_partial_rows(M2, groups, c)
        p2 = _f32(groups * R2 * c * 2, x)
        call("td_bn_fwd_partials", z2, z2.dtype, M2, groups, c, p2)
        z3 = _empty_cl(Nb, Cout, Ho, Wo, x, torch.bfloat16)
        a2 = _empty_cl(Nb, c, Ho, Wo, x, torch.bfloat16)
        S3 = lib.td_conv1x1_stat_rows(M2, groups, Cout)
        p3 = _f32(groups * S3 * Cout * 2, x)
        mean2, invstd2 = _f32(groups * c, x), _f32(groups * c, x)
        call("td_conv1x1_fwd_bnrelu", z2, w3, M2, groups, c, Cout, p2, R2, g2, b2, st2.running_mean, st2.running_var, st2.momentum,
             st2.eps, mean2, invstd2, a2, z3, p3)
        # identity branch
        zd = meand = invstdd = None
        if wd is not None:
            zd, pd, Sd = _conv1x1_stats(x, wd, groups, stride)
            shortcut, meand, invstdd = _bn_apply(zd, pd, Sd, gd, bd, std, None, False, groups)
        else:
            shortcut = x
        y, mean3, invstd3 = _bn_apply(z3, p3, S3, g3, b3, st3, shortcut, True, groups)
        ctx.save_for_backward(x, w1, w2, w3, g1, b1, g2, b2, g3, b3, wd, gd, bd, z1, a1, z2, a2, z3, y, zd, mean1, invstd1,
                              mean2, invstd2, mean3, invstd3, meand, invstdd)
        ctx.groups, ctx.stride = groups, stride
        return y

    @staticmethod
    def backward(ctx, dy):
        with wgrad_group():      # the node's 1x1 weight gradients leave as one grouped launch at the end
            return _Bottleneck._backward(ctx, dy)

    @staticmethod
    def _backward(ctx, dy):
        lib = native.load()
        (x, w1, w2, w3, g1, b1, g2, b2, g3, b3, wd, gd, bd, z1, a1, z2, a2, z3, y, zd, mean1, invstd1, mean2, invstd2, mean3,
         invstd3, meand, invstdd) = ctx.saved_tensors
        groups, stride = ctx.groups, ctx.stride
        Nb, Cin, H, W = x.shape
        c, Cout = w1.shape[0], w3.shape[0]
        Ho, Wo = z2.shape[2], z2.shape[3]
        M1, M2 = Nb * H * W, Nb * Ho * Wo
        BF = torch.bfloat16
        dy = _cl(dy, BF)

        wgrad = conv1x1_wgrad          # immediate, or enqueued inside deferred_wgrads()

        # bn3 (+ relu, + identity): dz3 and the identity branch's gradient (dy masked by the block's relu)
        dz3, dres, dg3, db3 = _bn_backward(dy, z3, y, g3, b3, mean3, invstd3, True, True, groups)
        # conv3: data gradient with bn2's backward sums in the epilogue; weight gradient against relu(bn2(z2))
        da2 = torch.empty_like(z2, memory_format=_CL)
        S2 = lib.td_conv1x1_stat_rows(M2, groups, c)
        q2 = _f32(groups * S2 * c * 2, x)
        call("td_conv1x1_dgrad_bnsums", dz3, w3, M2, groups, Cout, c, z2, g2, b2, mean2, invstd2, da2, q2)
        dw3 = wgrad(dz3, a2, w3, M2, c, Cout, Ho, Wo, 1)
        # bn2 dx from those sums
        dz2 = torch.empty_like(z2, memory_format=_CL)
        dg2, db2 = _f32(c, x), _f32(c, x)
        call("td_bn_bwd_from_partials", da2, z2, None, BF, g2, b2, mean2, invstd2, 1, M2, groups, c, q2, S2, dz2, None, dg2, db2)
        # conv2: MIOpen -- except the weight gradient of the shapes where the hand-written 3x3 kernel is ahead of MIOpen's
        # split-K kernel + its zero-fill / cast passes (profiles/r04/conv3x3_wgrad_bench_v2.txt: 64 -> 64 channels at 48 x 160)
        own_wgrad = conv3x3_wgrad_wins(Nb, Ho, Wo, c, c, stride)
        da1, dw2, _ = torch.ops.aten.convolution_backward(dz2, a1, w2, None, [stride, stride], [1, 1], [1, 1], False, [0, 0], 1,
                                                          [True, not own_wgrad, False])
        if own_wgrad:
            dw2 = conv3x3_wgrad(dz2, a1, w2, pad=1)
        da1 = _cl(da1)
        # bn1 statistics pass; its dx rides on conv1's data gradient
        R1 = lib.td_bn_partial_rows(M1, groups, c)
        q1 = _f32(groups * R1 * c * 2, x)
        call("td_bn_bwd_partials", da1, z1, None, BF, g1, b1, mean1, invstd1, 1, M1, groups, c, q1)
        # identity branch: x itself, or the down-sample convolution + bn
        dwd = dgd = dbd = None
        if wd is not None:
            dzd, _, dgd, dbd = _bn_backward(dres, zd, None, gd, bd, meand, invstdd, False, False, groups)
            if stride == 1:
                res_in = torch.empty_like(x, memory_format=_CL)
                call("td_conv1x1_dgrad", dzd, wd, M2, groups, Cout, Cin, None, res_in)
            else:      # strided 1x1: the gradient lands on every stride-th pixel (MIOpen writes the zeros in between)
                res_in = _cl(torch.ops.aten.convolution_backward(dzd, x, wd, None, [stride, stride], [0, 0], [1, 1], False, [0, 0],
                                                                 1, [True, False, False])[0], BF)
            dwd = wgrad(dzd, x, wd, M2, Cin, Cout, H, W, stride)
        else:
            res_in = dres
        dx = torch.empty_like(x, memory_format=_CL)
        dz1 = torch.empty_like(z1, memory_format=_CL)
        dg1, db1 = _f32(c, x), _f32(c, x)
        call("td_conv1x1_dgrad_bnbwd", da1, z1, w1, M1, groups, c, Cin, q1, R1, g1, b1, mean1, invstd1, dg1, db1, dz1, res_in, dx)
        dw1 = wgrad(dz1, x, w1, M1, Cin, c, H, W, 1)
        cast = lambda t, like: None if t is None else t.to(like.dtype)
        return (dx, dw1, dw2, dw3, cast(dg1, g1), cast(db1, b1), cast(dg2, g2), cast(db2, b2), cast(dg3, g3), cast(db3, b3),
                dwd, cast(dgd, gd) if gd is not None else None, cast(dbd, bd) if bd is not None else None,
                None, None, None, None, None, None)


def bottleneck_supported(x, w1, w2, w3, g1, wd=None, stride=1):
    c = w1.shape[0]
    return (_cl_tensor(x, 64, _BF16) and _weight_1x1_ok(w1) and _weight_1x1_ok(w3)
            and w2.dtype == torch.bfloat16 and w2.is_contiguous(memory_format=_CL) and g1.dtype == torch.float32
            and c % 64 == 0 and c <= 512 and w3.shape[0] % 64 == 0 and stride in (1, 2)
            and tuple(w1.shape[1:]) == (x.shape[1], 1, 1) and tuple(w3.shape[1:]) == (c, 1, 1) and tuple(w2.shape) == (c, c, 3, 3)
            and (wd is None or (_weight_1x1_ok(wd) and tuple(wd.shape) == (w3.shape[0], x.shape[1], 1, 1)))
            and (wd is not None or (stride == 1 and w3.shape[0] == x.shape[1])))


def bottleneck(x, w1, bn1, w2, bn2, w3, bn3, wd=None, bnd=None, groups=1, stride=1):
    """relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) + shortcut(x)) in training mode (reference: resnet.py:66-86), one
    autograd node over the fused kernels; bn* are the BatchNorm modules (affine parameters differentiable, running statistics
    updated in place)."""
    if x.shape[0] % groups:
        raise ValueError("batch %d is not %d stacked passes" % (x.shape[0], groups))
    if not bottleneck_supported(x, w1, w2, w3, bn1.weight, wd, stride):
        raise native.NativeLibraryError("bottleneck needs bf16 channels_last HIP tensors, channels % 64 == 0, planes <= 512")
    return _Bottleneck.apply(x, w1, w2, w3, bn1.weight, bn1.bias, bn2.weight, bn2.bias, bn3.weight, bn3.bias, wd,
                             bnd.weight if bnd is not None else None, bnd.bias if bnd is not None else None,
                             BnState(bn1), BnState(bn2), BnState(bn3), BnState(bnd) if bnd is not None else None, groups, stride)


def batchnorm_act_supported(x, weight):
    return _cl_tensor(x, 64) and weight is not None and weight.dtype == torch.float32


def batchnorm_act(x, weight, bias, running_mean, running_var, momentum, eps, residual=None, relu=False, groups=1):
    """Training-mode BatchNorm2d + optional residual add + optional ReLU (reference: resnet.py:30-49, 66-86).
    ``groups`` > 1: the batch is that many stacked passes, each normalised with its own batch statistics."""
    if x.shape[0] % groups:
        raise ValueError("batch %d is not %d stacked passes" % (x.shape[0], groups))
    if not batchnorm_act_supported(x, weight):
        raise native.NativeLibraryError("batchnorm_act needs a channels_last f32/bf16 HIP tensor with C % 64 == 0")
    return _BatchNormAct.apply(x, weight, bias, running_mean, running_var, _residual(residual, x), momentum, eps, relu, groups)


class _SyncBatchNormAct(torch.autograd.Function):
    """_BatchNormAct with the per-channel statistics summed over a process group between the two kernel stages."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, residual, momentum, eps, relu, groups, process_group):
        import torch.distributed as dist
        N, C, H, W = x.shape
        M = N * H * W
        packed = _f32(groups * C * 2 + 1, x)      # sums + row count: ONE collective
        ws = _f32(native.load().td_bn_workspace_floats(M, groups, C), x)
        call("td_bn_sync_fwd_sums", x, x.dtype, M, groups, C, packed, ws)
        packed[-1:].fill_(float(M // groups))
        dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=process_group)
        y = torch.empty_like(x, memory_format=_CL)
        mean, invstd = _f32(groups * C, x), _f32(groups * C, x)
        call("td_bn_sync_fwd_apply", x, residual, x.dtype, packed, packed[-1:], weight, bias, running_mean, running_var,
             float(momentum), float(eps), int(relu), M, groups, C, y, mean, invstd)
        ctx.save_for_backward(x, y if (relu and residual is not None) else None, weight, bias, mean, invstd, packed[-1:].clone())
        ctx.relu, ctx.has_res, ctx.groups, ctx.group = bool(relu), residual is not None, groups, process_group
        return y

    @staticmethod
    def backward(ctx, dy):
        import torch.distributed as dist
        x, y, weight, bias, mean, invstd, count = ctx.saved_tensors
        N, C, H, W = x.shape
        M = N * H * W
        G = ctx.groups
        dy = _cl(dy, x.dtype)
        local = _f32(G * C * 2, x)
        ws = _f32(native.load().td_bn_workspace_floats(M, G, C), x)
        call("td_bn_sync_bwd_sums", dy, x, y, x.dtype, weight, bias, mean, invstd, int(ctx.relu), M, G, C, local, ws)
        total = local.clone()
        dist.all_reduce(total, op=dist.ReduceOp.SUM, group=ctx.group)
        dx = torch.empty_like(x, memory_format=_CL)
        buf, dres = _dres(x, dy, ctx.has_res, ctx.relu)
        dgamma, dbeta, coef = _f32(C, x), _f32(C, x), _f32(G * C * 3, x)
        call("td_bn_sync_bwd_dx", dy, x, y, x.dtype, local, total, count, weight, bias, mean, invstd, int(ctx.relu), M, G, C, dx, buf,
             dgamma, dbeta, coef)
        return dx, dgamma.to(weight.dtype), dbeta.to(weight.dtype), None, None, dres, None, None, None, None, None


def sync_batchnorm_act(x, weight, bias, running_mean, running_var, momentum, eps, process_group, residual=None, relu=False,
                       groups=1):
    """batchnorm_act with batch statistics over ALL ranks of ``process_group`` (the reference's syncbn=True,
    mono/apis/trainer.py:156-157): one all-reduce of 2*groups*C+1 floats each way, the passes over the activation
    in the same hand-written kernels as the local form."""
    if x.shape[0] % groups:
        raise ValueError("batch %d is not %d stacked passes" % (x.shape[0], groups))
    if not batchnorm_act_supported(x, weight):
        raise native.NativeLibraryError("sync_batchnorm_act needs a channels_last f32/bf16 HIP tensor with C % 64 == 0")
    return _SyncBatchNormAct.apply(x, weight, bias, running_mean, running_var, _residual(residual, x), momentum, eps, relu, groups,
                                   process_group)


def edge_weights(img_at_scale, a, scale6):
    """Per-pixel, per-term image weights scale_k * exp(-a * mean_c |d_k I|) -> [B,6,h,w] (no gradient)."""
    img = _f32c(img_at_scale.detach())
    B, _, h, w = img.shape
    out = torch.empty(B, 6, h, w, device=img.device, dtype=torch.float32)
    call("td_edge_weights", img, B, h, w, float(a), (ctypes.c_float * 6)(*[float(v) for v in scale6]), out)
    return out


class _FeatReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, Wt):
        B, C, h, w = feat.shape
        nblk = native.load().td_featreg_num_blocks(B, h, w, C)
        partial, loss = _f32(nblk, feat), _f32(1, feat)
        call("td_featreg_fwd", feat, feat.dtype, Wt, B, h, w, C, partial)
        call("td_sum_scaled", partial, nblk, 1.0, loss)
        ctx.save_for_backward(feat, Wt)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        feat, Wt = ctx.saved_tensors
        B, C, h, w = feat.shape
        grad = torch.empty_like(feat, memory_format=_CL)
        call("td_featreg_bwd", feat, feat.dtype, Wt, _f32c(g.reshape(1)), B, h, w, C, grad)
        return grad, None


def featreg_supported(feat):
    return _cl_tensor(feat, 8) and feat.shape[2] >= 3 and feat.shape[3] >= 3


def feature_regularization(feat, img_at_scale, dis, cvt):
    """-dis * smooth1 + cvt * smooth2 of get_feature_regularization_loss
    (mono/model/mono_fm_joint/net.py:309-330) on a channels_last feature map, fused."""
    B, C, h, w = feat.shape
    n = float(B * C)
    counts = [n * h * (w - 1), n * (h - 1) * w, n * h * (w - 2), n * (h - 1) * (w - 1), n * (h - 1) * (w - 1),
              n * (h - 2) * w]
    coef = [-dis, -dis, cvt, cvt, cvt, cvt]
    Wt = edge_weights(img_at_scale, 1.0, [c / k for c, k in zip(coef, counts)])
    return _FeatReg.apply(feat, Wt)


class _ReconSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, hole):
        B, _, h, w = x.shape
        n = native.load().td_recon_num_tasks(B, h, w)
        partial, out = _f32(n, x), _f32(1, x)
        call("td_recon_fwd", x, y, hole, B, h, w, partial)
        call("td_sum_scaled", partial, n, 1.0, out)
        ctx.save_for_backward(x, y, hole)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        x, y, hole = ctx.saved_tensors
        B, _, h, w = x.shape
        dx = torch.empty_like(x)
        call("td_recon_bwd", x, y, hole, _f32c(g.reshape(1)), B, h, w, dx)
        return dx, None, None


def masked_reconstruction_sum(pred, target, hole):
    """sum_p hole[p] * (0.85 * mean_c SSIM(pred, target) + 0.15 * mean_c robust_l1) with gradient to
    ``pred`` (mono/model/mono_fm_joint_inpaint/net.py:84-89).  pred/target [B,3,h,w], hole [B,h,w]."""
    if pred.shape[2] < 3 or pred.shape[3] < 3:
        raise native.NativeLibraryError("masked_reconstruction_sum needs h, w >= 3")
    pred = pred.float().contiguous()          # (channels-last bf16 decoder output -> planar f32)
    return _ReconSum.apply(pred, _f32c(target.detach()), _f32c(hole.detach()))


def _pad_fwd(name, x, Ho, Wo):
    N, C, H, W = x.shape
    out = _empty_cl(N, C, Ho, Wo, x)
    call(name, x, x.dtype, N, H, W, C, out)
    return out


def _pad_bwd(name, g, H, W):
    N, C = g.shape[:2]
    g = _cl(g)
    gin = _empty_cl(N, C, H, W, g)
    call(name, g, g.dtype, N, H, W, C, gin)
    return gin


class _ReflPad1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _pad_fwd("td_reflpad1_fwd", x, x.shape[2] + 2, x.shape[3] + 2)

    @staticmethod
    def backward(ctx, g):
        return _pad_bwd("td_reflpad1_bwd", g, g.shape[2] - 2, g.shape[3] - 2)


class _Up2ReflPad1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _pad_fwd("td_up2_reflpad1_fwd", x, 2 * x.shape[2] + 2, 2 * x.shape[3] + 2)

    @staticmethod
    def backward(ctx, g):
        return _pad_bwd("td_up2_reflpad1_bwd", g, (g.shape[2] - 2) // 2, (g.shape[3] - 2) // 2)


def up2_reflpad1_supported(x):
    return _cl_tensor(x, 8)


def up2_reflpad1(x):
    """ReflectionPad2d(1)(interpolate(x, scale_factor=2, mode="nearest")) on a channels_last HIP tensor
    (reference: decoder.py:40-57)."""
    if not up2_reflpad1_supported(x):
        raise native.NativeLibraryError("up2_reflpad1 needs a channels_last f32/bf16 HIP tensor with C % 8 == 0")
    return _Up2ReflPad1.apply(x)


def reflpad1_supported(x):
    return _cl_tensor(x, 8) and x.shape[2] >= 2 and x.shape[3] >= 2


def reflpad1(x):
    """nn.ReflectionPad2d(1) on a channels_last HIP tensor (reference: layers.py:171-184)."""
    if not reflpad1_supported(x):
        raise native.NativeLibraryError("reflpad1 needs a channels_last f32/bf16 HIP tensor with C % 8 == 0")
    return _ReflPad1.apply(x)


class _FeatureWarpLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tgt_f, disp, P, invK, min_depth, max_depth, *src_f):
        B, C, h, w = tgt_f.shape
        hs, ws = disp.shape[2], disp.shape[3]
        dev = tgt_f.device
        n_src = len(src_f)
        disp = _f32c(disp)
        P = _f32c(P)
        argmin = torch.empty(B, h, w, device=dev, dtype=torch.uint8)
        nblk = native.load().td_featwarp_num_blocks(B, h, w)
        partial, loss = _f32(nblk, tgt_f), _f32(1, tgt_f)
        call("td_featwarp_fwd", tgt_f, src_f, n_src, tgt_f.dtype, disp, P, invK, B, h, w, C, hs, ws, float(min_depth),
             float(max_depth), argmin, partial)
        inv_count = 1.0 / float(B * h * w)
        call("td_sum_scaled", partial, nblk, inv_count, loss)
        ctx.save_for_backward(tgt_f, disp, P, invK, argmin, *src_f)
        ctx.meta = (min_depth, max_depth, inv_count, nblk)
        ctx.mark_non_differentiable(argmin)
        return loss.reshape(()), argmin

    @staticmethod
    def backward(ctx, g, _g_idx):
        tgt_f, disp, P, invK, argmin, *src_f = ctx.saved_tensors
        min_depth, max_depth, inv_count, nblk = ctx.meta
        B, C, h, w = tgt_f.shape
        hs, ws = disp.shape[2], disp.shape[3]
        dev = tgt_f.device
        n_src = len(src_f)
        gs = _f32c(g.reshape(1))
        d_tgt = torch.empty_like(tgt_f, memory_format=_CL)
        # int32 fixed-point accumulators of the scatter (integer atomics: order-independent, bit-reproducible)
        d_src32 = [torch.zeros((B, h, w, C), device=dev, dtype=torch.int32) for _ in src_f]
        d_up = torch.empty(B, h, w, device=dev, dtype=torch.float32)
        dP_part = torch.empty(nblk, n_src * 12, device=dev, dtype=torch.float32)
        call("td_featwarp_bwd", tgt_f, src_f, n_src, tgt_f.dtype, disp, P, invK, argmin, gs, inv_count, B, h, w, C, hs, ws,
             float(min_depth), float(max_depth), d_tgt, d_src32, d_up, dP_part)
        d_disp = torch.empty_like(disp)
        call("td_upsample_adjoint", d_up, B, h, w, hs, ws, d_disp, 0)
        dP = torch.empty_like(P)
        call("td_reduce_partials", dP_part, n_src, B, nblk // B, dP)
        # accumulators -> the gradient in the feature dtype, logical NCHW view of channels-last memory
        d_src = []
        for acc in d_src32:
            out = torch.empty((B, h, w, C), device=dev, dtype=tgt_f.dtype)
            call("td_featwarp_dsrc_finish", acc, gs, inv_count, C, acc.numel(), tgt_f.dtype, out)
            d_src.append(out.permute(0, 3, 1, 2))
        return (d_tgt, d_disp, dP, None, None, None) + tuple(d_src)


def featwarp_supported(tgt_f, src_f):
    return _cl_tensor(tgt_f, 64) and all(_cl_tensor(s, 64) and s.dtype == tgt_f.dtype and s.shape == tgt_f.shape for s in src_f) \
        and 1 <= len(src_f) <= 2 and tgt_f.shape[2] >= 2 and tgt_f.shape[3] >= 2


def feature_warp_min_loss(tgt_f, src_f, disp, P, invK, min_depth, max_depth):
    """mean over pixels of min_f mean_c sqrt((tgt_f - warp_f(src_f))^2 + 1e-6): generate_features_pred +
    compute_perceptional_loss + min over frames (reference: mono_fm_joint/net.py:196-223,63-65;
    mono_fm_joint_inpaint/net.py:58-70).  P / invK are at the feature resolution.
    Returns (loss, argmin uint8 [B,h,w])."""
    return _FeatureWarpLoss.apply(tgt_f, disp, P, _f32c(invK), min_depth, max_depth, *src_f)


class _RobustL1Map(torch.autograd.Function):
    # pred / dpred are of ANY dense layout (the kernel gets the strides), which native.call would refuse: hence _raw

    @staticmethod
    def forward(ctx, pred, target, weight):
        B, C, H, W = pred.shape
        out = torch.empty(B, 1, H, W, device=pred.device, dtype=torch.float32)
        call("td_l1map_fwd", _raw(pred), pred.dtype, native.strides_array(pred), target, B, C, H, W, float(weight), out)
        ctx.save_for_backward(pred, target)
        ctx.weight = float(weight)
        return out

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        B, C, H, W = pred.shape
        g = _f32c(g)                                         # (an expanded mean-gradient becomes a dense map here)
        dpred = torch.empty_strided(pred.size(), pred.stride(), device=pred.device, dtype=pred.dtype)
        call("td_l1map_bwd", _raw(pred), pred.dtype, native.strides_array(pred), target, g, B, C, H, W, ctx.weight, _raw(dpred))
        return dpred, None, None


def robust_l1_map_supported(pred, target):
    return (pred.is_cuda and pred.dim() == 4 and pred.dtype in native.DTYPE_CODES and target.shape == pred.shape
            and pred.shape[1] <= 64 and torch.ops.aten.is_non_overlapping_and_dense(pred))


def robust_l1_map(pred, target, weight=1.0):
    """weight * mean_c sqrt((pred - target)^2 + 1e-6) -> [B,1,H,W]: compute_perceptional_loss between a decoder
    output (any dense layout, f32/bf16, read in place) and an image (reference: compute_auto_res_loss,
    mono_fm_joint_inpaint/net.py:520-527; compute_colorization_loss, :310-323).  Gradient to ``pred`` only."""
    if not robust_l1_map_supported(pred, target):
        raise native.NativeLibraryError("robust_l1_map needs a dense f32/bf16 HIP prediction and a same-shape target")
    return _RobustL1Map.apply(pred, _f32c(target.detach()), weight)


def rgb2lab(rgb, l_cent=50.0, l_norm=50.0, ab_norm=110.0):
    """Normalised Lab of an sRGB image batch [B,3,H,W] (reference: color_conversions.py:106-114); no gradient."""
    rgb = _f32c(rgb.detach())
    B, C, H, W = rgb.shape
    if C != 3:
        raise ValueError("rgb2lab expects 3 channels")
    lab = torch.empty_like(rgb)
    call("td_rgb2lab", rgb, B, H, W, float(l_cent), float(l_norm), float(ab_norm), lab)
    return lab


class _PoseTransforms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, axisangle, translation, K, invert):
        n = len(invert)
        B = axisangle.shape[0] // n
        T = torch.empty(n, B, 4, 4, device=axisangle.device, dtype=torch.float32)
        P = torch.empty(n, B, 3, 4, device=axisangle.device, dtype=torch.float32)
        call("td_pose_fwd", axisangle, translation, native.int_array(invert), K, n, B, T, P)
        ctx.save_for_backward(axisangle, translation, K)
        ctx.invert = tuple(invert)
        return T, P

    @staticmethod
    def backward(ctx, gT, gP):
        axisangle, translation, K = ctx.saved_tensors
        n = len(ctx.invert)
        B = axisangle.shape[0] // n
        ga, gt = torch.empty_like(axisangle), torch.empty_like(translation)
        gT_c = _f32c(gT) if gT is not None else None      # converted copies stay alive across the launch
        gP_c = _f32c(gP) if gP is not None else None
        call("td_pose_bwd", axisangle, translation, native.int_array(ctx.invert), K, n, B, gT_c, gP_c, ga, gt)
        return ga, gt, None, None


def pose_transforms(axisangle, translation, K, invert):
    """All frame pairs of a step at once: (T [n,B,4,4], P [n,B,3,4] = (K @ T)[:, :3, :]) from the PoseDecoder's
    pair-major outputs axisangle / translation [n*B,3] (reference: transformation_from_parameters,
    mono_fm_joint/net.py:225-277; Project.forward's K @ T, layers.py:73-75).  ``invert[i]``: frame id < 0."""
    a = _f32c(axisangle.reshape(-1, 3))
    t = _f32c(translation.reshape(-1, 3))
    if a.shape[0] % len(invert):
        raise ValueError("pose rows %d are not %d pairs of equal batch" % (a.shape[0], len(invert)))
    return _PoseTransforms.apply(a, t, _f32c(K), [bool(v) for v in invert])


def color_jitter_expand(frames_u8, aug):
    """uint8 frames [N,3,H,W] + per-image jitter parameters [N,9] -> (color, color_aug) float32 [N,3,H,W]
    (reference: ToTensor + ColorJitter in MonoDataset.preprocess, mono/datasets/mono_dataset.py:83-101)."""
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[1] != 3:
        raise ValueError("frames_u8 must be uint8 [N,3,H,W]")
    frames_u8 = frames_u8.contiguous()
    aug = _f32c(aug)
    N, _, H, W = frames_u8.shape
    if aug.shape != (N, 9):
        raise ValueError("aug must be [N,9]")
    color = torch.empty(N, 3, H, W, device=frames_u8.device, dtype=torch.float32)
    color_aug = torch.empty_like(color)
    scratch = _f32(N, frames_u8)
    call("td_color_jitter", frames_u8, aug, N, H, W, scratch, color, color_aug)
    return color, color_aug


def quantize_fp8(t):
    """Per-tensor current-scaling fp8 quantisation of a dense f32/bf16 HIP tensor: (q float8_e4m3fn with t's shape,
    inv_scale [1] float32 with t ~= q * inv_scale).  Two launches, no host round trip (csrc/td_fp8.hip)."""
    if not (t.is_cuda and t.dtype in native.DTYPE_CODES and t.numel() % 8 == 0 and torch.ops.aten.is_non_overlapping_and_dense(t)):
        raise native.NativeLibraryError("quantize_fp8 needs a dense f32/bf16 HIP tensor with numel % 8 == 0")
    n = t.numel()
    partials = _f32(native.load().td_fp8_num_blocks(n), t)
    q = torch.empty_strided(t.size(), t.stride(), device=t.device, dtype=torch.uint8)
    inv_scale = _f32(1, t)
    # t / q are of ANY dense layout (the kernels run over the memory in storage order), checked above: hence _raw
    call("td_fp8_amax_partials", _raw(t), t.dtype, n, partials)
    call("td_fp8_quantize", _raw(t), t.dtype, n, partials, _raw(q), inv_scale)
    return q.view(torch.float8_e4m3fn), inv_scale


class _Conv1x1FP8(torch.autograd.Function):
    """y = conv2d(x, w[, b]) for a 1x1 stride-1 convolution on channels-last activations, forward GEMM in fp8 on the MFMA
    (hipBLASLt through torch._scaled_mm, fp32 accumulation, bf16 out); backward in the activation dtype from the
    saved full-precision operands."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        N, C, H, W = x.shape
        K = weight.shape[0]
        w = weight.to(x.dtype).contiguous(memory_format=torch.channels_last)
        xq, sx = quantize_fp8(x)
        wq, sw = quantize_fp8(w)
        a = xq.permute(0, 2, 3, 1).reshape(N * H * W, C)                 # [M, Cin] row-major view of the NHWC memory
        b = wq.reshape(K, C).t()                                         # [Cin, Cout] column-major
        y = torch._scaled_mm(a, b, scale_a=sx, scale_b=sw, bias=bias.to(x.dtype) if bias is not None else None,
                             out_dtype=x.dtype)
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.wdtype = weight.dtype
        return y.reshape(N, H, W, K).permute(0, 3, 1, 2)                 # logical NCHW, channels-last memory

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.to(x.dtype).contiguous(memory_format=torch.channels_last)
        gx, gw, gb = torch.ops.aten.convolution_backward(gy, x, w, [w.shape[0]] if ctx.has_bias else None, [1, 1], [0, 0], [1, 1],
                                                          False, [0, 0], 1, [True, True, ctx.has_bias])
        return gx, gw.to(ctx.wdtype), (gb.to(ctx.wdtype) if ctx.has_bias else None)


def conv1x1_fp8_supported(x, weight):
    return (_cl_tensor(x, 16, _BF16) and weight.dim() == 4 and weight.shape[2:] == (1, 1) and weight.shape[1] == x.shape[1]
            and weight.shape[0] % 16 == 0 and hasattr(torch, "float8_e4m3fn"))


def conv1x1_fp8(x, weight, bias=None):
    """1x1 stride-1 convolution with the forward GEMM on the fp8 MFMA path (BASELINE config 5); see _Conv1x1FP8."""
    if not conv1x1_fp8_supported(x, weight):
        raise native.NativeLibraryError("conv1x1_fp8 needs a channels_last bf16 HIP activation, Cin % 16 == Cout % 16 == 0")
    return _Conv1x1FP8.apply(x, weight, bias)
