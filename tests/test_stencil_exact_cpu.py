"""The cases of tests/test_hip_stencil_exact.py without a GPU: the replicas of the launch geometry in tests/stencil_exact_util.py are
held against the library's host functions (td_smooth_num_blocks, td_featreg_num_blocks, td_recon_num_tasks load on a CPU-only
machine) at every case, every case's data meets the preconditions its tier rests on (exact sums; no zero term and both signs in the
no-zero fields; zero terms in the zero-rich ones; both weights and a single-channel step per term in the binary images; 18 pairwise
different weights around every pixel of the caller-made Wt), and the float64 references ARE the operation: they agree with
oracle/smooth.py and oracle/photometric.py under torch autograd in double to float64 round-off before either judges a kernel."""
import pytest
import torch

from oracle import photometric, smooth
from tests import stencil_exact_util as E

RTOL = 1e-12
F64 = torch.float64


def _lib():
    import tripled_amd  # noqa: F401
    from tripled_amd import native
    return native.load()


def _close(got, ref, what):
    assert float((got - ref).abs().max()) <= RTOL * max(1.0, float(ref.abs().max())), what


def _id(shape):
    return "x".join(map(str, shape))


# ---- the launch geometry ------------------------------------------------------------------------------------------------------------------

def test_replicas_agree_with_the_library():
    lib = _lib()
    for B, h, w in E.EDGE_SHAPES + ((0, 3, 3), (1, 16, 64), (1, 17, 65)):
        assert lib.td_smooth_num_blocks(B, h, w) == E.smooth_num_blocks(B, h, w)
    for B, C, h, w in E.FEATREG_SHAPES:
        assert lib.td_featreg_num_blocks(B, h, w, C) == E.featreg_num_blocks(B, h, w, C)
    for B, h, w in E.RECON_SHAPES:
        assert lib.td_recon_num_tasks(B, h, w) == E.recon_geometry(B, h, w, E.RC_FWD_COLS).ntasks


def test_smoothness_shapes_reach_the_tile_edges():
    grids = {s: E.smooth_grid(s[1], s[2]) for s in E.SMOOTH_SHAPES}
    assert {g[0] for g in grids.values()} == {1, 2, 3} and {g[1] for g in grids.values()} == {1, 2, 3}
    over = lambda n, t: n - (E._cdiv(n, t) - 1) * t          # anchors in the last tile
    assert {over(s[2], E.ST_W) for s in E.SMOOTH_SHAPES} >= {1, 2, 3, 64} and {over(s[1], E.ST_H) for s in E.SMOOTH_SHAPES} >= {1, 2, 3, 16}
    assert max(s[0] for s in E.SMOOTH_SHAPES) == 3
    v = torch.arange(2 * 17 * 65, dtype=F64).reshape(2, 17, 65)
    ts = E.tile_sums(v)                                       # block (b gy + by) gx + bx
    assert ts.numel() == 8 and float(ts[5]) == float(v[1, :16, 64:].sum()) and float(ts[2]) == float(v[0, 16:, :64].sum())
    threads = [B * h * w for B, h, w in E.EDGE_SHAPES]
    assert 2 * 5 * 257 in threads and 86 * 3 in threads and all(t % E.TD_THREADS for t in threads)


def test_feature_regulariser_shapes_reach_the_block_edges():
    threads = {s: s[0] * s[2] * s[3] * (s[1] // 8) for s in E.FEATREG_SHAPES}
    assert threads[(1, 8, 16, 16)] == 256 and threads[(1, 8, 3, 86)] == 258 and threads[(3, 24, 17, 9)] == 1377
    # C / 8 = 3: 256 is no multiple of 3, so the three channel vectors of pixel 85 straddle blocks 0 and 1, and a sample's 459
    # threads end inside a block
    assert E.featreg_thread(255, 17, 9, 24) == (0, 9, 4, 0) and E.featreg_thread(256, 17, 9, 24) == (0, 9, 4, 1)
    assert E.featreg_thread(459, 17, 9, 24) == (1, 0, 0, 0)
    B, C, h, w = 3, 24, 17, 9
    v = torch.arange(B * C * h * w, dtype=F64).reshape(B, C, h, w)
    sums = E.featreg_block_sums(v)
    by_thread = torch.zeros_like(sums)
    for gid in range(B * h * w * (C // 8)):
        b, y, x, cv = E.featreg_thread(gid, h, w, C)
        by_thread[gid // E.TD_THREADS] += v[b, cv * 8:cv * 8 + 8, y, x].sum()
    assert torch.equal(sums, by_thread)


def test_area_cases_reach_every_group_size():
    seen = {}
    for fy, fx in E.AREA_FACTORS:
        n = fy * fx
        seen.setdefault(E.area_group(n), set()).add(n % E.area_group(n) != 0)
    # a window that G divides and one that it does not (the ragged `e += G` loop), for every G that has lanes to share
    assert seen == {1: {False}, 4: {False, True}, 16: {False, True}, 64: {False, True}}
    assert [E.area_group(n) for n in (15, 16, 63, 64, 255, 256)] == [1, 4, 4, 16, 16, 64]
    assert any(fy == 1 and fx > 1 for fy, fx in E.AREA_FACTORS) and any(fy != fx for fy, fx in E.AREA_FACTORS)
    totals = [B * C * h * w for B, C, h, w in E.AREA_OUTPUTS]
    assert totals == [1, 45, 630]
    for G in (4, 16, 64):       # a lone group in a block; blocks whose last group is dead; waves whose groups lie in two planes
        assert all((t * G) % E.TD_THREADS for t in totals)
    assert (7 * 9) % 16 and (7 * 9) % 4 and (7 * 9) % 1 == 0


def test_recon_cases_reach_the_strip_edges():
    geo = {s: (E.recon_geometry(*s, E.RC_FWD_COLS), E.recon_geometry(*s, E.RC_BWD_COLS)) for s in E.RECON_SHAPES}
    assert geo[(1, 10, 61)][1].last == 1 and geo[(2, 16, 63)][0].last == 1           # one live column in the last strip
    assert geo[(1, 17, 121)][1].last == 1 and geo[(5, 17, 125)][0].last == 1 and geo[(1, 17, 121)][0].last == 59
    f = geo[(5, 17, 125)][0]
    assert (f.ntasks, f.blocks, f.grid) == (45, 12, 16)                              # four idle blocks after the XCD remap
    assert geo[(5, 17, 125)][1].nstrips == 3 and geo[(5, 17, 125)][1].last == 5
    assert all(g[0].nchunks == E._cdiv(s[1], 8) for s, g in geo.items())


# ---- the preconditions of the data ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", tuple(dict.fromkeys(E.EDGE_SHAPES + tuple((s[0],) + s[2:] for s in E.FEATREG_SHAPES))), ids=_id)
def test_binary_images_offer_both_weights_and_single_channel_steps(shape):
    img = E.binary_image(*shape)
    assert set(img.unique().tolist()) == {0.0, E.STEP}
    r = E.binary_image_report(img)
    for k, name in enumerate(E.TERMS):
        assert r.zeros[k] > 0 and r.ones[k] > 0, name              # both weights, inside the term's domain
        assert r.single[k] > 0, name                               # a step that one channel alone carries
    assert r.pairs
    for a in (0.5, 1.0):        # exactly 0 or 1 in float32: the argument is -0 or below -170, the smallest denormal is e^-103.3
        m = E.image_terms(img)
        assert float((a * m[m > 0] / 3).min()) > 170.0
    wt = E.edge_weights_ref(E.binary_weights(img), E.SCALE6)
    dom = E.domains(*shape[1:])
    assert not bool(wt.permute(1, 0, 2, 3)[~dom[:, None].expand(6, shape[0], *shape[1:])].any())
    assert len(set(E.SCALE6)) == 6 and E.SCALE6[0] < 0 and E.SCALE6[1] < 0


@pytest.mark.parametrize("shape", E.SMOOTH_SHAPES, ids=_id)
def test_no_zero_fields_have_no_zero_term_and_both_signs(shape):
    B, h, w = shape
    d = E.nozero_disp(B, h, w)
    units = E.six_terms(d) / E.DISP_UNIT
    dom = E.domains(h, w)[:, None].expand(6, B, h, w)
    assert torch.equal(units, units.round()) and float(d.min()) >= E.DISP_UNIT and float(d.max()) <= 1.0
    for k, name in enumerate(E.TERMS):
        t = units[k][dom[k]]
        assert float(t.abs().min()) >= 1.0, name                    # no zero term: at least one unit
        if t.numel() >= 16:
            assert 0.25 <= float((t > 0).double().mean()) <= 0.75, name
    # the sign margin: a computed term is off by < 8 u max|d inv|, one unit is 2^-6 inv
    assert E.TERM_ROUNDINGS * E.U * float(d.max()) * 2 ** 14 <= E.DISP_UNIT
    E.mean_inv_f32(d)


def test_no_zero_field_at_the_size_the_construction_was_checked_at():
    units = E.six_terms(E.nozero_disp(1, 40, 140)) / E.DISP_UNIT
    dom = E.domains(40, 140)[:, None]
    for k in range(6):
        t = units[k][dom[k]]
        assert int((t == 0).sum()) == 0 and 0.4 < float((t > 0).double().mean()) < 0.6
        assert set((t % 8).unique().tolist()) <= ({1.0, 3.0, 5.0, 7.0}, {1.0, 3.0, 5.0, 7.0}, {2.0}, {4.0}, {4.0}, {2.0})[k]


@pytest.mark.parametrize("shape", E.SMOOTH_SHAPES, ids=_id)
def test_zero_rich_fields_hold_zero_terms_and_exact_sums(shape):
    B, h, w = shape
    c = E.smooth_case(B, h, w, "zero")                 # its builder asserts check_exact on every sum the kernels form
    dom = E.domains(h, w)[:, None].expand(6, B, h, w)
    for k, name in enumerate(E.TERMS):
        t = c.raw[k][dom[k]]
        if h * w > 9 or k not in (3, 4):               # a 3 x 3 map has no room for a flat 2 x 2 block next to its zero row and column
            assert int((t == 0).sum()) > 0, name
        if t.numel() >= 16:
            assert bool((t > 0).any()) and bool((t < 0).any()), name
    assert bool((c.disp == 0).all(2).any()) and bool((c.disp == 0).all(1).any())          # a row and a column of zeros
    assert torch.equal(c.inv, torch.ones(B, dtype=F64)) and torch.equal(c.d, c.g)
    assert torch.equal(c.partial.float().double(), c.partial)


@pytest.mark.parametrize("shape", E.FEATREG_SHAPES, ids=_id)
def test_caller_made_weights_are_pairwise_different_around_every_pixel(shape):
    B, C, h, w = shape
    c = E.featreg_case(B, C, h, w)                     # asserts the exactness of every block sum and of the gradient
    gw = E.gathered_weights(c.Wt)
    assert len(E.GATHERS) == 18
    for i in range(18):
        for j in range(i + 1, 18):
            assert not bool((gw[i] == gw[j]).any()), (E.GATHERS[i], E.GATHERS[j])         # NaN (no such anchor) equals nothing
    dom = E.domains(h, w)[None].expand(B, 6, h, w)
    assert not bool(c.Wt[~dom].any()) and bool((c.Wt[dom] != 0).all())
    assert bool((c.Wt[:, :2][dom[:, :2]] < 0).all()) and bool((c.Wt[:, 2:][dom[:, 2:]] > 0).all())
    assert {0.25, 0.5, 1.0, 2.0} <= set(c.Wt.abs().unique().tolist())
    assert 16.0 < float(c.feat.abs().max()) <= 32.0 and c.partial.numel() == c.nblk


# ---- the float64 references are the operation ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("image", ("binary", "dyadic"))
@pytest.mark.parametrize("normalize", (True, False))
@pytest.mark.parametrize("shape", ((1, 3, 3), (2, 17, 64), (3, 33, 130)), ids=_id)
def test_smoothness_reference_agrees_with_the_oracle_under_autograd(shape, normalize, image):
    B, h, w = shape
    disp = E.nozero_disp(B, h, w)                      # no zero term: autograd of |.| is unambiguous
    img = (E.binary_image if image == "binary" else E.dyadic_image)(B, h, w)
    w6 = E.binary_weights(img) if image == "binary" else E.exp_weights(img, 0.5)
    inv = 1.0 / (disp.mean((1, 2)) + 1e-7) if normalize else torch.ones(B, dtype=F64)
    ref = E.smooth_core(disp, w6, inv, normalize, E.SMOOTH_WEIGHT, E.SMOOTH_GSCALE * E.SMOOTH_WEIGHT)
    d = disp[:, None].clone().requires_grad_(True)
    loss = E.SMOOTH_WEIGHT * smooth.smooth_loss(smooth.mean_normalize(d) if normalize else d, img.double())
    (loss * E.SMOOTH_GSCALE).backward()
    assert abs(float(loss.detach()) - ref.loss) <= RTOL * abs(ref.loss)
    _close(d.grad[:, 0], ref.d, "d_disp")
    assert bool((ref.T >= ref.g.abs()).all())


@pytest.mark.parametrize("shape", ((1, 8, 3, 3), (2, 24, 3, 5), (3, 24, 17, 9)), ids=_id)
def test_feature_regulariser_reference_agrees_with_the_oracle_under_autograd(shape):
    B, C, h, w = shape
    c = E.featreg_case(B, C, h, w)
    img = E.dyadic_image(B, h, w)
    scale = [k / n for k, n in zip((-c.dis, -c.dis, c.cvt, c.cvt, c.cvt, c.cvt), E.counts(B * C, h, w))]
    Wt = (E.exp_weights(img, 1.0) * torch.tensor(scale, dtype=F64)[:, None, None, None]).permute(1, 0, 2, 3)
    fwd, _, grad, mag = E.featreg_refs(c.feat, Wt, E.FEATREG_GSCALE)
    f = c.feat.clone().requires_grad_(True)
    loss = smooth.feature_regularization_loss(f, img.double(), c.dis, c.cvt)
    (loss * E.FEATREG_GSCALE).backward()
    assert abs(float(loss.detach()) - float(fwd.sum())) <= RTOL * float(fwd.abs().sum())
    _close(f.grad, grad, "grad")
    assert bool((mag >= grad.abs()).all())


def test_edge_weight_reference_is_the_oracles_weight():
    img = E.dyadic_image(2, 5, 7)
    for a in (0.5, 1.0):
        w6 = E.exp_weights(img, a)
        i_dx, i_dy = smooth.gradient(img.double())
        i_dxx, i_dxy = smooth.gradient(i_dx)
        i_dyx, i_dyy = smooth.gradient(i_dy)
        for k, t in enumerate((i_dx, i_dy, i_dxx, i_dxy, i_dyx, i_dyy)):
            ref = torch.exp(-a * t.abs().mean(1))
            _close(w6[k][:, :ref.shape[1], :ref.shape[2]], ref, E.TERMS[k])
            assert int((w6[k] != 0).sum()) == ref.numel()                # and 0 outside the domain


def test_area_reference_is_the_area_mean():
    for fy, fx in ((3, 5), (7, 9), (17, 16)):
        c = E.area_case(fy, fx, 2, 5, 7, 9)
        ref = smooth.area_resize(c.img.double(), 7, 9)
        assert float((c.out.double() - ref).abs().max()) <= 2.0 ** -24 and c.G == E.area_group(fy * fx)
    for n in E.SUM_SCALED_N:
        p, out = E.sum_scaled_case(n)
        assert float(out) == 0.5 * float(p.double().sum())


@pytest.mark.parametrize("shape", ((1, 3, 3), (2, 16, 63)), ids=_id)
def test_recon_reference_agrees_with_the_oracle_under_autograd(shape):
    c = E.recon_case(*shape)
    x = c.x.double().requires_grad_(True)
    ref = torch.sum(photometric.reprojection_loss(x, c.y.double())[:, 0] * c.hole.double())
    (ref * 0.5).backward()
    assert abs(c.S - float(ref.detach())) <= RTOL * abs(float(ref.detach()))
    _close(c.grad, x.grad, "d S / d x")
    ring = torch.ones(shape[1], shape[2], dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    assert bool((c.hole[:, ring] >= 1).all())
