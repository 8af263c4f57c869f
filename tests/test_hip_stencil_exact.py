"""The edge-aware stencil kernels (csrc/td_smooth.hip, csrc/td_featreg.hip) and the strip edges of csrc/td_recon.hip through the C ABI,
on fields for which everything around the exp and the |.| is exact (tests/stencil_exact_util.py: the fields, the tiers, the derived
bounds and the one stated assumption; their preconditions are proven in tests/test_stencil_exact_cpu.py).  Bit-exact tiers compare
element by element (-0 equals +0) and name the first element that differs: for the smoothness partials that is a block and a term.
Every bounded comparison holds AT EVERY ELEMENT -- no pixel is exempt -- and prints the largest observed fraction of its bound.

Every operand lies between NaN guard rows; every output of an ABI call is NaN inside marker guard rows: afterwards no NaN is left and
no guard row was touched.  (The one end-to-end run of ops.feature_regularization writes to buffers the binding allocates.)"""
import ctypes
import types

import pytest
import torch

from tests import stencil_exact_util as E

pytestmark = pytest.mark.gpu

F32 = torch.float32
DTYPES = pytest.mark.parametrize("dt", (F32, E.BF), ids=("f32", "bf16"))


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _native():
    import tripled_amd  # noqa: F401
    from tripled_amd import native
    return native.load(), native


def _first(bad):
    return tuple(int(i) for i in torch.nonzero(bad)[0])


def _same(got, ref, what):
    got = got.detach().cpu()
    ref = ref.reshape(got.shape).to(got.dtype)
    bad = ~(got == ref)                                  # a NaN is a difference
    if bool(bad.any()):
        i = _first(bad)
        raise AssertionError("%s: %d of %d elements differ, the first at %s: %r, expected %r"
                             % (what, int(bad.sum()), bad.numel(), i, float(got[i]), float(ref[i])))


def _bounded(got, ref, bnd, what):
    got = got.detach().double().cpu().reshape(ref.shape)
    bnd = bnd if isinstance(bnd, torch.Tensor) else torch.full_like(ref, bnd)
    err = (got - ref).abs()
    live = bnd > 0
    print("%s: largest error / bound %.3f" % (what, float((err[live] / bnd[live]).max()) if bool(live.any()) else 0.0))
    bad = ~(err <= bnd)
    if bool(bad.any()):
        i = _first(bad)
        raise AssertionError("%s: %d of %d elements outside the bound, the first at %s: %r, expected %r +- %.3e"
                             % (what, int(bad.sum()), bad.numel(), i, float(got[i]), float(ref[i]), float(bnd[i])))


def _scalar(v):
    return E.guard(torch.tensor([[v]], dtype=F32))


def _t(v):
    return torch.tensor([v], dtype=torch.float64)


# ---- the replicas of the launch geometry against the library -------------------------------------------------------------------------

def test_geometry_replicas_agree_with_the_library():
    lib, _ = _native()
    for B, h, w in E.EDGE_SHAPES:
        assert lib.td_smooth_num_blocks(B, h, w) == E.smooth_num_blocks(B, h, w)
    for B, C, h, w in E.FEATREG_SHAPES:
        assert lib.td_featreg_num_blocks(B, h, w, C) == E.featreg_num_blocks(B, h, w, C)
    for B, h, w in E.RECON_SHAPES:
        assert lib.td_recon_num_tasks(B, h, w) == E.recon_geometry(B, h, w, E.RC_FWD_COLS).ntasks


# ---- td_area_downsample, td_sum_scaled: bit-exact ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("out", E.AREA_OUTPUTS, ids=_id)
@pytest.mark.parametrize("f", E.AREA_FACTORS, ids=_id)
def test_area_downsample_is_one_rounded_division_of_the_exact_sum(f, out):
    _, native = _native()
    (fy, fx), (B, C, h, w) = f, out
    c = E.area_case(fy, fx, B, C, h, w)
    img = E.guard(c.img)
    runs = []
    for _ in range(2):
        o = E.guard_out((B, C, h, w))
        native.call("td_area_downsample", img, B, C, h * fy, w * fx, h, w, o.t)
        torch.cuda.synchronize()
        E.assert_guard(o, "area mean")
        runs.append(o.t.cpu())
    _same(runs[0], c.out, "area mean, %d x %d window, G = %d" % (fy, fx, c.G))
    assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("n", E.SUM_SCALED_N)
def test_sum_scaled_is_exact_on_dyadic_partials(n):
    _, native = _native()
    p, ref = E.sum_scaled_case(n)
    o = E.guard_out((1, 1))
    native.call("td_sum_scaled", E.guard(p.reshape(1, n)), n, 0.5, o.t)
    torch.cuda.synchronize()
    E.assert_guard(o, "td_sum_scaled")
    _same(o.t, ref, "td_sum_scaled")


# ---- smoothness -------------------------------------------------------------------------------------------------------------------------------

def _smooth_run(c):
    """Forward, finish, backward (accumulate = 0) and backward again with accumulate = 1 into integers; every buffer fenced."""
    _, native = _native()
    B, h, w = c.B, c.h, c.w
    disp, img, gscale = E.guard(c.disp.float()), E.guard(c.img), _scalar(E.SMOOTH_GSCALE)
    o = types.SimpleNamespace(mean=E.guard_out((1, B)), partial=E.guard_out((c.nblk, 6)), loss=E.guard_out((1, 1)),
                              g_hat=E.guard_out((B, h, w)), dot=E.guard_out((1, c.nblk)), d=E.guard_out((B, h, w)))
    native.call("td_smooth_fwd", disp, img, B, h, w, c.normalize, o.mean.t, o.partial.t)
    native.call("td_smooth_finish", o.partial.t, B, h, w, E.SMOOTH_WEIGHT, o.loss.t)
    native.call("td_smooth_bwd", disp, img, o.mean.t, B, h, w, c.normalize, gscale, E.SMOOTH_WEIGHT, o.g_hat.t, o.dot.t, o.d.t, 0)
    o.prefill = torch.randint(-8, 9, (B, h, w), generator=E._gen("prefill", B, h, w)).float()
    o.acc, o.g_hat2, o.dot2 = E.guard_out((B, h, w), init=o.prefill), E.guard_out((B, h, w)), E.guard_out((1, c.nblk))
    native.call("td_smooth_bwd", disp, img, o.mean.t, B, h, w, c.normalize, gscale, E.SMOOTH_WEIGHT, o.g_hat2.t, o.dot2.t, o.acc.t, 1)
    torch.cuda.synchronize()
    for name in ("mean", "partial", "loss", "g_hat", "dot", "d", "acc", "g_hat2", "dot2"):
        E.assert_guard(getattr(o, name), name)
    return o


def _check_smooth(c, o, what):
    _same(o.mean.t, c.mean, what + " mean[b]")
    if c.normalize:
        _bounded(o.partial.t, c.partial, c.e_partial, what + " partial[block][term]")
    else:
        _same(o.partial.t, c.partial, what + " partial[block][term]")
    _bounded(o.loss.t, _t(c.loss), _t(c.e_loss), what + " loss")
    _bounded(o.g_hat.t, c.g, c.e_g, what + " g_hat")
    if c.normalize:
        _bounded(o.dot.t, c.dot, c.e_dot, what + " dot_partial[block]")
        _bounded(o.d.t, c.d, c.e_d, what + " d_disp")
    else:
        _same(o.d.t, o.g_hat.t.cpu(), what + " d_disp == g_hat")
    # accumulate = 1: the pre-fill plus the accumulate = 0 result, one rounding; the workspaces do not depend on it
    _same(o.acc.t, o.prefill + o.d.t.cpu(), what + " accumulate")
    _same(o.g_hat2.t, o.g_hat.t.cpu(), what + " g_hat of the second run")
    _same(o.dot2.t, o.dot.t.cpu(), what + " dot_partial of the second run")


@pytest.mark.parametrize("mode", ("zero", "nozero"))
@pytest.mark.parametrize("shape", E.SMOOTH_SHAPES, ids=_id)
def test_smoothness_with_binary_weights(shape, mode):
    """normalize = 0 on zero-rich fields: partials, mean bit-exact, sign(0) = 0, d_disp == g_hat.  normalize = 1 on no-zero fields:
    mean bit-exact, everything else within the derived bounds of float64 evaluated with the kernel's own float inv."""
    c = E.smooth_case(*shape, mode)
    _check_smooth(c, _smooth_run(c), "%s %s" % (_id(shape), mode))


def test_smoothness_with_a_dyadic_image():
    c = E.smooth_case(3, 33, 130, "nozero-dyadic")
    _check_smooth(c, _smooth_run(c), "3x33x130 dyadic image")


# ---- td_edge_weights --------------------------------------------------------------------------------------------------------------------------

def _edge_weights(img, a):
    _, native = _native()
    B, _, h, w = img.shape
    o = E.guard_out((B, 6, h, w))
    native.call("td_edge_weights", E.guard(img), B, h, w, a, (ctypes.c_float * 6)(*E.SCALE6), o.t)
    torch.cuda.synchronize()
    E.assert_guard(o, "Wt")
    return o.t.cpu()


@pytest.mark.parametrize("a", (1.0, 0.5))
@pytest.mark.parametrize("shape", E.EDGE_SHAPES, ids=_id)
def test_edge_weights_of_a_binary_image_are_the_scale_or_zero(shape, a):
    img = E.binary_image(*shape)
    got = _edge_weights(img, a)
    outside = ~E.domains(*shape[1:])[None].expand(shape[0], 6, *shape[1:])
    _same(got[outside], torch.zeros(int(outside.sum())), "Wt where the term has no anchor")       # the backward relies on these zeros
    _same(got, E.edge_weights_ref(E.binary_weights(img), E.SCALE6), "Wt[b][term][y][x]")


@pytest.mark.parametrize("a", (1.0, 0.5))
@pytest.mark.parametrize("shape", E.EDGE_SHAPES, ids=_id)
def test_edge_weights_of_a_dyadic_image_within_eight_u(shape, a):
    img = E.dyadic_image(*shape)
    ref = E.edge_weights_ref(E.exp_weights(img, a), E.SCALE6)
    _bounded(_edge_weights(img, a), ref, E.W_REL * E.U * ref.abs(), "Wt %s a = %g" % (_id(shape), a))


# ---- feature regulariser ----------------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("shape", E.FEATREG_SHAPES, ids=_id)
def test_feature_regulariser_from_caller_made_weights_is_exact(shape, dt):
    _, native = _native()
    B, C, h, w = shape
    c = E.featreg_case(B, C, h, w)
    feat, Wt = E.guard(c.feat.permute(0, 2, 3, 1), dt), E.guard(c.Wt.float())
    partial, grad = E.guard_out((1, c.nblk)), E.guard_out((B, h, w, C), dt)
    native.call("td_featreg_fwd", feat, dt, Wt, B, h, w, C, partial.t)
    native.call("td_featreg_bwd", feat, dt, Wt, _scalar(E.FEATREG_GSCALE), B, h, w, C, grad.t)
    torch.cuda.synchronize()
    E.assert_guard(partial, "partial")
    E.assert_guard(grad, "grad")
    _same(partial.t, c.partial, "partial[block]")
    ref = c.grad.permute(0, 2, 3, 1)
    _same(grad.t, E.bf(ref) if dt == E.BF else ref, "grad[b][y][x][channel]")         # bf16: float64 rounded once


@DTYPES
@pytest.mark.parametrize("shape", E.FEATREG_SHAPES, ids=_id)
def test_feature_regularization_end_to_end_under_a_binary_image(shape, dt):
    import tripled_amd  # noqa: F401
    from tripled_amd import ops
    B, C, h, w = shape
    c = E.featreg_case(B, C, h, w)
    f = E.guard(c.feat.permute(0, 2, 3, 1), dt).permute(0, 3, 1, 2).requires_grad_(True)
    loss = ops.feature_regularization(f, E.guard(c.img), c.dis, c.cvt)
    (loss * E.FEATREG_GSCALE).backward()
    _bounded(loss.detach().reshape(1), _t(c.loss2), _t(c.e_loss2), "loss")
    bnd = c.e_grad2 + (E.bf16_half_spacing(c.grad2) if dt == E.BF else 0.0)
    _bounded(f.grad, c.grad2, bnd, "grad")


# ---- masked reconstruction at the strip edges -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", E.RECON_SHAPES, ids=_id)
def test_masked_reconstruction_at_the_strip_edges(shape):
    lib, native = _native()
    B, h, w = shape
    c = E.recon_case(B, h, w)
    n = lib.td_recon_num_tasks(B, h, w)
    assert n == c.fwd.ntasks
    x, y, hole = E.guard(c.x), E.guard(c.y), E.guard(c.hole)
    partial, S, dx = E.guard_out((1, n)), E.guard_out((1, 1)), E.guard_out((B, 3, h, w))
    native.call("td_recon_fwd", x, y, hole, B, h, w, partial.t)
    native.call("td_sum_scaled", partial.t, n, 1.0, S.t)
    native.call("td_recon_bwd", x, y, hole, _scalar(0.5), B, h, w, dx.t)
    torch.cuda.synchronize()
    for o, name in ((partial, "partial"), (S, "S"), (dx, "dx")):
        E.assert_guard(o, name)
    # the tolerances of tests/test_hip_recon.py: the project's own numbers (fast rcp / sqrt, the SSIM adjoint's conditioning)
    _bounded(S.t, _t(c.S), _t(1e-5 * max(1.0, abs(c.S))), "S")
    _bounded(dx.t, c.grad, 2e-3 * float(c.grad.abs().max()), "dS/dx, element by element")
    assert float((dx.t.double().cpu() - c.grad).abs().max() / c.grad.abs().max()) < 2e-3
