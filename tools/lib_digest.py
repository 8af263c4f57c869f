#!/usr/bin/env python
"""SHA-256 of every output buffer of the BatchNorm, 1x1 GEMM, join, max-pool and l1-map entry points on seeded Gaussian data, through
whichever build of the library TD_HIP_LIB names (default: this tree's).  Two builds compute the same bits exactly when the two
outputs of this program are the same file:

    TD_HIP_LIB=<parent>/lib/libtripled_hip.so python tools/lib_digest.py > digest_parent.txt
    python tools/lib_digest.py > digest_head.txt && cmp digest_parent.txt digest_head.txt

One line per entry point and case: ``entry-point case sha256``, the hash taken over every output buffer of the call (each under its
name, in a fixed order); a BatchNorm case is a shape and a dtype, hashed over its five relu / residual / mask variants.  Workspaces and
scratch (partials after their consumer, coef) are left out.
The shapes are small and reach each path of the host layer: BatchNorm row splits below / above the shrink threshold (96 rows) and at
the 512 cap, wide short layers cut into 16 ranges, groups 1 ... 3; strided and plain GEMM rows; single and grouped weight gradients.
"""
import ctypes
import hashlib
import os
import sys
import zlib

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tripled_amd  # noqa: E402,F401
from tripled_amd import native  # noqa: E402

DEV = "cuda:0"
DTYPES = (("bf16", torch.bfloat16), ("f32", torch.float32))


def randn(case, name, *shape, dtype=torch.float32, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(zlib.crc32(("%s/%s" % (case, name)).encode()))
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype).to(DEV)


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def absorb(h, tag, **buffers):
    torch.cuda.synchronize()
    h.update(tag.encode())
    for name, t in buffers.items():      # every output buffer of the call, in this order, each under its name
        if t is not None:
            h.update(name.encode() + b"\0" + t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())


def emit(entry, case, **buffers):
    h = hashlib.sha256()
    absorb(h, "", **buffers)
    print(entry, case, h.hexdigest())


def batchnorm(lib):
    for Mg, G, C in ((129, 3, 64), (1026, 1, 512), (6145, 1, 64), (32770, 2, 64)):
        M = Mg * G
        ws_floats, rows = lib.td_bn_workspace_floats(M, G, C), lib.td_bn_partial_rows(M, G, C)
        for dname, dt in DTYPES:
            # one line per entry point, shape and dtype: the hash runs over the five variants (relu, residual, mask from y); without
            # y the mask is re-derived from x, which no residual form allows
            hashes = {}
            for relu, residual, from_y in ((0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 1), (1, 0, 0)):
                case = "Mg%d_G%d_C%d_%s_relu%d_res%d_%s" % (Mg, G, C, dname, relu, residual, "y" if from_y else "x")
                emit = lambda entry, case, **buffers: absorb(hashes.setdefault(entry, hashlib.sha256()), case, **buffers)
                x = randn(case, "x", M, C, dtype=dt, shift=0.3)
                res = randn(case, "res", M, C, dtype=dt) if residual else None
                dy = randn(case, "dy", M, C, dtype=dt)
                gamma, beta = randn(case, "gamma", C, shift=1.0, scale=0.3), randn(case, "beta", C, scale=0.3)
                new_stats = lambda: (zeros(G, C), zeros(G, C), zeros(C), torch.ones(C, device=DEV))
                ws = lambda: zeros(ws_floats)

                y, (mean, invstd, rmean, rvar) = zeros(M, C, dtype=dt), new_stats()
                native.call("td_bn_fwd", x, res, dt, gamma, beta, rmean, rvar, 0.1, 1e-5, relu, M, G, C, y, mean, invstd, ws())
                emit("td_bn_fwd", case, y=y, save_mean=mean, save_invstd=invstd, running_mean=rmean, running_var=rvar)
                y_in = y if from_y else None

                part = zeros(G, rows, C, 2)
                native.call("td_bn_fwd_partials", x, dt, M, G, C, part)
                emit("td_bn_fwd_partials", case, partials=part)
                y2, (mean2, invstd2, rmean2, rvar2) = zeros(M, C, dtype=dt), new_stats()
                native.call("td_bn_fwd_from_partials", x, res, dt, gamma, beta, rmean2, rvar2, 0.1, 1e-5, relu, M, G, C, part, rows, y2,
                            mean2, invstd2)
                emit("td_bn_fwd_from_partials", case, y=y2, save_mean=mean2, save_invstd=invstd2, running_mean=rmean2, running_var=rvar2)

                outs = lambda: (zeros(M, C, dtype=dt), zeros(M, C, dtype=dt) if residual else None, zeros(C), zeros(C))
                dx, dres, dgamma, dbeta = outs()
                native.call("td_bn_bwd", dy, x, y_in, dt, gamma, beta, mean, invstd, relu, M, G, C, dx, dres, dgamma, dbeta, ws())
                emit("td_bn_bwd", case, dx=dx, dresidual=dres, dgamma=dgamma, dbeta=dbeta)

                part = zeros(G, rows, C, 2)
                native.call("td_bn_bwd_partials", dy, x, y_in, dt, gamma, beta, mean, invstd, relu, M, G, C, part)
                emit("td_bn_bwd_partials", case, partials=part)
                dx, dres, dgamma, dbeta = outs()
                native.call("td_bn_bwd_from_partials", dy, x, y_in, dt, gamma, beta, mean, invstd, relu, M, G, C, part, rows, dx, dres,
                            dgamma, dbeta)
                emit("td_bn_bwd_from_partials", case, dx=dx, dresidual=dres, dgamma=dgamma, dbeta=dbeta)

                # the synchronised forms of one rank: global sums = local sums, count = the rows of a group
                sums, count = zeros(G, C, 2), torch.full((1,), float(Mg), device=DEV)
                native.call("td_bn_sync_fwd_sums", x, dt, M, G, C, sums, ws())
                emit("td_bn_sync_fwd_sums", case, sums=sums)
                y3, (mean3, invstd3, rmean3, rvar3) = zeros(M, C, dtype=dt), new_stats()
                native.call("td_bn_sync_fwd_apply", x, res, dt, sums, count, gamma, beta, rmean3, rvar3, 0.1, 1e-5, relu, M, G, C, y3, mean3,
                            invstd3)
                emit("td_bn_sync_fwd_apply", case, y=y3, save_mean=mean3, save_invstd=invstd3, running_mean=rmean3, running_var=rvar3)
                bsums = zeros(G, C, 2)
                native.call("td_bn_sync_bwd_sums", dy, x, y_in, dt, gamma, beta, mean, invstd, relu, M, G, C, bsums, ws())
                emit("td_bn_sync_bwd_sums", case, sums=bsums)
                dx, dres, dgamma, dbeta = outs()
                native.call("td_bn_sync_bwd_dx", dy, x, y_in, dt, bsums, bsums, count, gamma, beta, mean, invstd, relu, M, G, C, dx, dres,
                            dgamma, dbeta, zeros(G, C, 3))
                emit("td_bn_sync_bwd_dx", case, dx=dx, dresidual=dres, dgamma=dgamma, dbeta=dbeta)
            for entry, h in hashes.items():
                print(entry, "Mg%d_G%d_C%d_%s" % (Mg, G, C, dname), h.hexdigest())


def gemm(lib):
    bf = torch.bfloat16
    # (images, Hi, Wi, stride) -> output rows M; stride 1: M rows, Hi = Wi = 0
    for case, M, rows_in, K, N, Hi, Wi, stride in (("s1", 777, 777, 128, 192, 0, 0, 1), ("s2", 2 * 5 * 6, 2 * 9 * 11, 64, 128, 9, 11, 2)):
        x, w = randn(case, "x", rows_in, K, dtype=bf), randn(case, "w", N, K, dtype=bf, scale=0.1)
        y, stat = zeros(M, N, dtype=bf), zeros(1, lib.td_conv1x1_stat_rows(M, 1, N), N, 2)
        native.call("td_conv1x1_fwd", x, w, M, 1, K, N, Hi, Wi, stride, y, stat)
        emit("td_conv1x1_fwd", case, y=y, stat_partials=stat)
    problems = ((777, 777, 128, 64, 0, 0, 1), (60, 198, 64, 128, 9, 11, 2), (5000, 5000, 256, 64, 0, 0, 1))      # M, rows_in, K, N, Hi, Wi, stride
    dys = [randn("wg%d" % i, "dy", p[0], p[3], dtype=bf) for i, p in enumerate(problems)]
    xs = [randn("wg%d" % i, "x", p[1], p[2], dtype=bf) for i, p in enumerate(problems)]
    work = lambda: [zeros(lib.td_conv1x1_wgrad_workspace_floats(p[0], p[2], p[3])) for p in problems]
    for dname, dt in DTYPES:
        for i, (M, _, K, N, Hi, Wi, stride) in enumerate(problems):
            dw = zeros(N, K, dtype=dt)
            native.call("td_conv1x1_wgrad", dys[i], xs[i], M, K, N, Hi, Wi, stride, dt, dw, work()[i])
            emit("td_conv1x1_wgrad", "p%d_%s" % (i, dname), dw=dw)
    col = lambda j: native.int_array([p[j] for p in problems])
    for gname, dts in (("bf16", [torch.bfloat16] * 3), ("f32", [torch.float32] * 3), ("mixed", [torch.float32, torch.bfloat16, torch.float32])):
        dws = [zeros(p[3], p[2], dtype=dt) for p, dt in zip(problems, dts)]
        native.call("td_conv1x1_wgrad_group", len(problems), dys, xs, (ctypes.c_longlong * 3)(*[p[0] for p in problems]), col(2), col(3),
                    col(4), col(5), col(6), native.int_array([native.DTYPE_CODES[dt] for dt in dts]), dws, work())
        emit("td_conv1x1_wgrad_group", gname, **{"dw%d" % i: dw for i, dw in enumerate(dws)})


def pointwise(lib):
    for dname, dt in DTYPES:
        npix, C0, C1, C2 = (1000, 16, 24, 3) if dname == "bf16" else (333, 8, 40, 8)
        a, b, tail = randn(dname, "a", npix, C0, dtype=dt), randn(dname, "b", npix, C1, dtype=dt), randn(dname, "t", npix, C2, dtype=dt)
        out = zeros(npix, C0 + C1 + 8, dtype=dt)
        native.call("td_join_fwd", a, b, tail, dt, npix, C0, C1, C2, out)
        emit("td_join_fwd", dname, out=out)
        ga, gb, gt = zeros(npix, C0, dtype=dt), zeros(npix, C1, dtype=dt), zeros(npix, C2, dtype=dt)
        native.call("td_join_bwd", randn(dname, "go", npix, C0 + C1 + 8, dtype=dt), dt, npix, C0, C1, C2, ga, gb, gt)
        emit("td_join_bwd", dname, grad_a=ga, grad_b=gb, grad_tail=gt)

        N, H, W = (2, 6, 10) if dname == "bf16" else (1, 14, 4)
        a, tail = randn(dname, "ua", N * H * W, C0, dtype=dt), randn(dname, "ut", N * H * W, C2, dtype=dt)
        b_half, out = randn(dname, "ub", N * (H // 2) * (W // 2), C1, dtype=dt), zeros(N * H * W, C0 + C1 + 8, dtype=dt)
        native.call("td_join_up2_fwd", a, b_half, tail, dt, N, H, W, C0, C1, C2, out)
        emit("td_join_up2_fwd", dname, out=out)
        ga, gb, gt = zeros(N * H * W, C0, dtype=dt), zeros(N * (H // 2) * (W // 2), C1, dtype=dt), zeros(N * H * W, C2, dtype=dt)
        native.call("td_join_up2_bwd", randn(dname, "ugo", N * H * W, C0 + C1 + 8, dtype=dt), dt, N, H, W, C0, C1, C2, ga, gb, gt)
        emit("td_join_up2_bwd", dname, grad_a=ga, grad_b_half=gb, grad_tail=gt)

        N, H, W, C = (2, 13, 17, 64) if dname == "bf16" else (1, 40, 41, 64)      # f32: the strip-scatter backward (H W >= 1536, C % 64 == 0)
        inp = randn(dname, "pool", N * H * W, C, dtype=dt)
        out, idx = zeros(N * H * W, C, dtype=dt), zeros(N * H * W, C, dtype=torch.uint8)
        native.call("td_maxpool5_fwd", inp, dt, N, H, W, C, out, idx)
        emit("td_maxpool5_fwd", dname, out=out, idx=idx)
        go, gi = randn(dname, "pgo", N * H * W, C, dtype=dt), zeros(N * H * W, C, dtype=dt)
        native.call("td_maxpool5_bwd", go, idx, dt, N, H, W, C, gi)
        emit("td_maxpool5_bwd", dname, grad_in=gi)
        gi = zeros(N * H * W, C, dtype=dt)
        native.call("td_maxpool5_bwd_add", go, idx, randn(dname, "padd", N * H * W, C, dtype=dt), dt, N, H, W, C, gi)
        emit("td_maxpool5_bwd_add", dname, grad_in=gi)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        out, idx = zeros(N * Ho * Wo, C, dtype=dt), zeros(N * Ho * Wo, C, dtype=torch.uint8)
        native.call("td_maxpool3s2_fwd", inp, dt, N, H, W, C, out, idx)
        emit("td_maxpool3s2_fwd", dname, out=out, idx=idx)
        gi = zeros(N * H * W, C, dtype=dt)
        native.call("td_maxpool3s2_bwd", randn(dname, "p3go", N * Ho * Wo, C, dtype=dt), idx, dt, N, H, W, C, gi)
        emit("td_maxpool3s2_bwd", dname, grad_in=gi)

        B, C, H, W = (2, 3, 12, 20) if dname == "bf16" else (3, 2, 7, 33)
        pred, target = randn(dname, "pred", B, C, H, W, dtype=dt), randn(dname, "target", B, C, H, W)
        out, dpred = zeros(B, 1, H, W), zeros(B, C, H, W, dtype=dt)
        native.call("td_l1map_fwd", pred, dt, native.strides_array(pred), target, B, C, H, W, 0.85, out)
        emit("td_l1map_fwd", dname, out=out)
        native.call("td_l1map_bwd", pred, dt, native.strides_array(pred), target, randn(dname, "gmap", B, 1, H, W), B, C, H, W, 0.85, dpred)
        emit("td_l1map_bwd", dname, dpred=dpred)


def main():
    assert torch.cuda.is_available(), "lib_digest.py needs cuda:0"
    torch.cuda.set_device(0)
    lib = native.load()
    batchnorm(lib)
    gemm(lib)
    pointwise(lib)
    return 0


if __name__ == "__main__":
    sys.exit(main())
