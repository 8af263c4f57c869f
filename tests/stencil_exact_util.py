"""Exact tests of the edge-aware stencil losses (csrc/td_smooth.hip, csrc/td_featreg.hip) and of the strip edges of csrc/td_recon.hip:
the field builders, float64 references, replicas of the launch geometry and fenced buffers that tests/test_stencil_exact_cpu.py (no
GPU) and tests/test_hip_stencil_exact.py share.  The technique is the one of tests/gemm_exact_util.py and tests/bn_exact_util.py
(check_exact, the generators and the fenced buffers are imported, not copied), adapted to a loss with an exp and an |.| in it: the
inputs are chosen so that everything AROUND the transcendental is exact and the sign of every stencil term is unambiguous.

dyadic fields   disparities are integers times 2^-6, features integers in [-32, 32] (exact in bf16), images multiples of 2^-8: every
                first and second difference, every per-tile sum of |term|, sum disp and every area-window sum is an fp32 value in any
                order (check_exact, stated on the reference alone).
binary weights  the image takes the values 0 and 1024 only, so a term's weight expf(-a m / 3) has m = 0 or m >= 1024: exactly 1
                (expf(-0.f)) or exactly 0 (e^-170 is far below the smallest float32 denormal).  The float64 reference therefore
                takes the weight as [m == 0], NOT as exp() in double, which would be 1e-74.
no-zero fields  d(y, x) = 8 r(y, x) + ((x^2 + y^2 + 4 x y) mod 8): modulo 8, dx and dy are odd, dxx and dyy are 2, dxy and dyx are 4,
                so no term is 0 and multiplying by the inexact 1 / (mean + 1e-7) of normalize = 1 cannot change a sign: one unit is
                2^-6 inv, a computed term is off by less than 8 u max|d inv| <= 8 u inv (u = 2^-24): a margin of 2^15.
zero-rich fields for normalize = 0 (inv = 1, every t exact): flat patches of at least 3 x 3 and a row and a column of zeros per
                sample, so many terms are exactly 0 and both sides must give sign(0) = 0.

Three tiers of assertion.  BIT-EXACT: the area mean (one correctly rounded float32 division of an exact sum), td_sum_scaled, the
per-sample mean, partial[block][term] of the smoothness forward with binary weights and normalize = 0, td_edge_weights on binary
images (scale6[k] or 0), partial[block] and grad of the feature regulariser from caller-made dyadic weights, accumulate = 1.
DERIVED BOUND (g(n) = n u / (1 - n u); the counts are roundings along the longest path of one addend):
  loss, exact partials     tot_k is exact; tot_k / cnt_k (1), total += (5), weight * (1):      |err| <= g(7) ref
  g_hat, binary weights    each of the <= 18 addends is +-{1,2} w icnt_k: icnt_k = (gscale weight) / (B h (w-1)) carries 3 roundings,
                           sign w icnt_k is exact for w in {0, 1}, the sum has <= 17 additions:  |err| <= g(20) sum |addend|  (G_C)
  g_hat, general weights   w itself is within W_REL = 8 u (below) and w icnt_k rounds once more: |err| <= g(29) sum |addend|
  a computed term, normalize = 1:  4 operands d inv (1 each), 2 first differences, 1 second difference of magnitude <= 2 M:
                           |t^ - t| <= 8 u M (1 + u), M = max |d inv| of the sample                                 (TERM_ROUNDINGS)
  partial, normalize = 1   |t^| w (1), 4 per-thread + 6 wave + 2 block additions (12): e_p = (1 + g(13 + W)) sum w 8 u M + g(13 + W) sum w |t|
  loss, normalize = 1      sum over blocks (8 levels), / cnt (1), total (5), weight (1):  weight sum_k [(1 + g(15)) sum e_p + g(15) sum p] / cnt_k
  dot_partial              g^ D (1), 12 additions: e_dot = (1 + g(13)) sum_tile |D| e_g + g(13) sum_tile |g D|
  d_disp, normalize = 1    corr = tot inv inv / n: 8 levels + 3: e_corr = [(1 + g(11)) sum e_dot + g(11) sum |dot|] inv^2 / n;
                           v = g^ inv - corr (2): (1 + g(2)) (inv e_g + e_corr) + g(2) (|g inv| + |corr|);  normalize = 0: d_disp == g_hat
  featreg end to end       Wt = scale_k {0, 1} with scale_k = float(coef_k / count_k), the reference uses that float: the loss has
                           1 product + 5 + 8 per-thread + 6 + 2 block + 1 + 8 + 1 finish = 32 roundings per addend, the gradient <= 17
                           additions + the product with gscale: g(32) sum |addend|, g(18) sum |addend| (+ half a bf16 spacing)
STATED ASSUMPTION: the device expf is taken as accurate to 3 ulp.  W_REL = 8 u relative for a weight on a dyadic image with
|arg| = a mean_c |d_k I| <= 1: m / 3 and the product with a move the argument by <= 2 u |arg| <= 2 u (amplified by exp to the same
relative error), the scale multiplies once (u), which leaves 5 u for expf itself.  Nothing on hand documents the device expf; the
GPU file prints the largest observed fraction of this bound.

Two wishes that cannot both be had (four weight values, and no two alike around a pixel): 18 (anchor, term) weights touch a pixel in the feature regulariser's
backward, and they can only be pairwise different if there are 18 values, so the caller-made Wt takes the magnitudes 0.25 (1 .. 18)
(0.25, 0.5, 1 and 2 among them), negative for the two first-order terms, zero outside each term's domain.  And since the image takes
two values only, an in-domain dx (dy) step always makes dxx (dyy) non-zero too: what the builders guarantee instead is that every
pair of terms but the mathematically identical dxy / dyx has an anchor where their weights differ.

The launch geometry of the kernel files is REPLICATED here (the 16 x 64 smoothness tile, the feature regulariser's thread -> (pixel,
channel vector) -> block map, area_downsample's choice of G, the strips, chunks and tasks of td_recon): a change of the tile sizes
or of G's thresholds in csrc/td_smooth.hip, csrc/td_featreg.hip or csrc/td_recon.hip must be mirrored here; the tests hold the
replicas against td_smooth_num_blocks, td_featreg_num_blocks and td_recon_num_tasks for every case.

Every builder is deterministic (seeded by its own arguments) and cached.  Nothing here touches a GPU at import."""
import collections
import functools
import types

import torch

from tests.bn_exact_util import U, bf16_half_spacing, f32  # noqa: F401
from tests.gemm_exact_util import BF, MARKER, NAN, _gen, assert_fence, bf, check_exact, fenced, fenced_input, fenced_output  # noqa: F401

F64 = torch.float64
ST_H, ST_W, TD_THREADS = 16, 64, 256            # csrc/td_smooth.hip, csrc/td_common.h
RC_ROWS, RC_WAVES, RC_FWD_COLS, RC_BWD_COLS = 8, 4, 62, 60      # csrc/td_recon.hip
DISP_UNIT, IMG_UNIT, STEP = 2.0 ** -6, 2.0 ** -8, 1024.0
TERMS = ("dx", "dy", "dxx", "dxy", "dyx", "dyy")
G_C, W_REL, TERM_ROUNDINGS = 20, 8, 8
SMOOTH_WEIGHT, SMOOTH_GSCALE = 0.25, 2.0
FEATREG_GSCALE = 0.5
SCALE6 = (-0.75, -1.5, 1.25, 0.625, 3.0, 0.375)         # six distinct dyadic scales, the first two negative as the caller passes them

SMOOTH_SHAPES = ((1, 3, 3), (2, 3, 64), (1, 4, 65), (1, 16, 66), (2, 17, 64), (1, 18, 129), (3, 33, 130), (1, 3, 129), (2, 33, 3))
EDGE_SHAPES = SMOOTH_SHAPES + ((2, 5, 257), (1, 86, 3))                 # 2570 and 258 threads: a ragged last block of the 1-D grid
FEATREG_SHAPES = ((1, 8, 3, 3), (2, 24, 3, 5), (1, 8, 16, 16), (1, 8, 3, 86), (3, 24, 17, 9), (1, 64, 6, 20))      # (B, C, h, w)
RECON_SHAPES = ((1, 10, 61), (2, 16, 63), (1, 17, 121), (5, 17, 125))
AREA_FACTORS = ((1, 1), (2, 2), (3, 5), (4, 4), (2, 8), (1, 16), (7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (17, 16), (32, 32))
AREA_OUTPUTS = ((1, 1, 1, 1), (1, 3, 3, 5), (2, 5, 7, 9))               # (B, C, h, w)
SUM_SCALED_N = (1, 255, 256, 257, 1000)


def gamma(n):
    return n * U / (1.0 - n * U)


def _cdiv(a, b):
    return -(-a // b)


# ---- replicas of the launch geometry ------------------------------------------------------------------------------------------------

def smooth_grid(h, w):
    return _cdiv(h, ST_H), _cdiv(w, ST_W)


def smooth_num_blocks(B, h, w):
    gy, gx = smooth_grid(h, w)
    return B * gy * gx if min(B, h, w) > 0 else 0


def tile_sums(v):
    """[B, h, w] float64 -> [B gy gx]: the sum over each 16 x 64 tile of anchors, in the order of the kernels' block index
    (b gy + by) gx + bx."""
    B, h, w = v.shape
    gy, gx = smooth_grid(h, w)
    p = torch.zeros(B, gy * ST_H, gx * ST_W, dtype=F64)
    p[:, :h, :w] = v
    return p.reshape(B, gy, ST_H, gx, ST_W).sum((2, 4)).reshape(-1)


def featreg_num_blocks(B, h, w, C):
    return _cdiv(B * h * w * (C // 8), TD_THREADS) if min(B, h, w, C) > 0 else 0


def featreg_thread(gid, h, w, C):
    """Global thread index -> (b, y, x, channel vector) of featreg_*_kernel."""
    c8 = C // 8
    pix = gid // c8
    return pix // (w * h), (pix // w) % h, pix % w, gid % c8


def featreg_block_sums(v):
    """[B, C, h, w] float64, one value per pixel and channel -> [blocks]: a thread owns 8 consecutive channels of a pixel of the
    channels-last memory and a block 256 consecutive threads, so a block owns 2048 consecutive elements of [B, h, w, C]."""
    B, C, h, w = v.shape
    n = featreg_num_blocks(B, h, w, C)
    p = torch.zeros(n * TD_THREADS * 8, dtype=F64)
    p[:v.numel()] = v.permute(0, 2, 3, 1).reshape(-1)
    return p.reshape(n, -1).sum(1)


def area_group(n):
    """Lanes per output of area_downsample_kernel<G> for a window of n elements."""
    return 64 if n >= 256 else 16 if n >= 64 else 4 if n >= 16 else 1


def area_blocks(total, G):
    return _cdiv(total * G, TD_THREADS)


def recon_geometry(B, h, w, cols):
    """Strips of `cols` output columns (62 forward, 60 backward), chunks of 8 rows, one wave per task, 4 waves per block, the grid
    rounded up to 8 XCDs."""
    nstrips, nchunks = _cdiv(w, cols), _cdiv(h, RC_ROWS)
    ntasks = B * nstrips * nchunks
    blocks = _cdiv(ntasks, RC_WAVES)
    return types.SimpleNamespace(nstrips=nstrips, nchunks=nchunks, ntasks=ntasks, blocks=blocks, grid=_cdiv(blocks, 8) * 8,
                                 last=w - (nstrips - 1) * cols)


# ---- the six stencil terms and their adjoint, float64 -----------------------------------------------------------------------------------

def six_terms(F):
    """F [..., h, w] float64 -> [6, ..., h, w]: term k anchored at (y, x); 0 where term k has no anchor."""
    T = torch.zeros((6,) + tuple(F.shape), dtype=F64)
    T[0][..., :, :-1] = F[..., :, 1:] - F[..., :, :-1]
    T[1][..., :-1, :] = F[..., 1:, :] - F[..., :-1, :]
    T[2][..., :, :-2] = F[..., :, 2:] - 2.0 * F[..., :, 1:-1] + F[..., :, :-2]
    mixed = F[..., 1:, 1:] - F[..., 1:, :-1] - F[..., :-1, 1:] + F[..., :-1, :-1]
    T[3][..., :-1, :-1] = mixed          # dx of the row below - dx
    T[4][..., :-1, :-1] = mixed          # dy of the column to the right - dy: the same four operands
    T[5][..., :-2, :] = F[..., 2:, :] - 2.0 * F[..., 1:-1, :] + F[..., :-2, :]
    return T


def domains(h, w):
    """[6, h, w] bool: the anchors of each term."""
    d = torch.zeros(6, h, w, dtype=torch.bool)
    d[0][:, :w - 1] = True
    d[1][:h - 1, :] = True
    d[2][:, :w - 2] = True
    d[3][:h - 1, :w - 1] = True
    d[4][:h - 1, :w - 1] = True
    d[5][:h - 2, :] = True
    return d


def counts(n, h, w):
    """Anchors of each term over n planes."""
    return [n * h * (w - 1), n * (h - 1) * w, n * h * (w - 2), n * (h - 1) * (w - 1), n * (h - 1) * (w - 1), n * (h - 2) * w]


def six_adjoint(S, magnitudes=False):
    """S [6, ..., h, w]: one coefficient per (term, anchor), 0 outside the term's domain -> [..., h, w]: sum over the <= 18 (anchor,
    term) pairs touching a pixel of coefficient x stencil entry (magnitudes: of |coefficient| |stencil entry|, the sum |addend|)."""
    n = -1.0
    if magnitudes:
        S, n = S.abs(), 1.0
    g = torch.zeros(tuple(S.shape[1:]), dtype=F64)
    s = S[0][..., :, :-1]
    g[..., :, 1:] += s
    g[..., :, :-1] += n * s
    s = S[1][..., :-1, :]
    g[..., 1:, :] += s
    g[..., :-1, :] += n * s
    s = S[2][..., :, :-2]
    g[..., :, 2:] += s
    g[..., :, 1:-1] += 2.0 * n * s
    g[..., :, :-2] += s
    for k in (3, 4):
        s = S[k][..., :-1, :-1]
        g[..., 1:, 1:] += s
        g[..., 1:, :-1] += n * s
        g[..., :-1, 1:] += n * s
        g[..., :-1, :-1] += s
    s = S[5][..., :-2, :]
    g[..., 2:, :] += s
    g[..., 1:-1, :] += 2.0 * n * s
    g[..., :-2, :] += s
    return g


def image_terms(img):
    """img [B, 3, h, w] -> m [6, B, h, w] = sum_c |term k of channel c| (exact for the images built here)."""
    return six_terms(img.double()).abs().sum(2)


def binary_weights(img):
    """[6, B, h, w]: the weights of a 0 / 1024 image, exactly 0 or 1 on the device for a >= 0.5; 0 outside the domain."""
    m = image_terms(img)
    assert bool(((m == 0) | (m >= STEP)).all())
    return (m == 0).double() * domains(*img.shape[2:])[:, None]


def exp_weights(img, a):
    """[6, B, h, w] float64 weights exp(-a mean_c |d_k I|) of a dyadic image, 0 outside the domain; |arg| <= 1 (W_REL)."""
    arg = a * image_terms(img) / 3.0
    assert float(arg.max()) <= 1.0
    return torch.exp(-arg) * domains(*img.shape[2:])[:, None]


def edge_weights_ref(w6, scale6):
    """Wt [B, 6, h, w] float64 from weights [6, B, h, w] and the float scale6."""
    s = torch.tensor([f32(v) for v in scale6], dtype=F64)
    return (w6 * s[:, None, None, None]).permute(1, 0, 2, 3).contiguous()


# ---- field builders -----------------------------------------------------------------------------------------------------------------------

def zero_rich_disp(B, h, w):
    """Integers in [0, 64) times 2^-6 with flat patches of at least 3 x 3 (when the map is larger than that) and, written last, a row
    and a column of zeros per sample."""
    g = _gen("zero-rich", B, h, w)
    d = torch.randint(0, 64, (B, h, w), generator=g).double()
    r = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    for b in range(B):
        for _ in range(max(1, h * w // 48) if h * w > 9 else 0):
            ph, pw = r(3, min(h, 6)), r(3, min(w, 9))
            y0, x0 = r(0, h - ph), r(0, w - pw)
            d[b, y0:y0 + ph, x0:x0 + pw] = r(0, 63)
        d[b, r(0, h - 1), :] = 0
        d[b, :, r(0, w - 1)] = 0
    return d * DISP_UNIT


def nozero_disp(B, h, w):
    """(d + 1) 2^-6 with d = 8 r + ((x^2 + y^2 + 4 x y) mod 8), r seeded integers in [0, 8): no stencil term is ever 0."""
    g = _gen("no-zero", B, h, w)
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    d = 8 * torch.randint(0, 8, (B, h, w), generator=g) + ((x * x + y * y + 4 * x * y) % 8)[None]
    return (d.double() + 1.0) * DISP_UNIT


def binary_image_report(img):
    """What a 0 / 1024 image offers, per term: anchors of weight 0, of weight 1, and anchors whose image derivative is non-zero in
    exactly one channel (dropping a channel from the mean turns that 0 into a 1); and whether every pair of terms (but dxy / dyx,
    which are the same expression) has an anchor, inside both domains, where the two weights differ."""
    h, w = img.shape[2:]
    dom = domains(h, w)[:, None]
    wt = binary_weights(img)
    single = ((six_terms(img.double()) != 0).sum(2) == 1) & dom
    pairs = all(bool(((wt[j] != wt[k]) & dom[j] & dom[k]).any()) for j in range(6) for k in range(j + 1, 6) if (j, k) != (3, 4))
    return types.SimpleNamespace(zeros=[int(((wt[k] == 0) & dom[k]).sum()) for k in range(6)], ones=[int(wt[k].sum()) for k in range(6)],
                                 single=[int(single[k].sum()) for k in range(6)], pairs=pairs)


def _report_ok(r):
    return min(r.zeros) > 0 and min(r.ones) > 0 and min(r.single) > 0 and r.pairs


@functools.lru_cache(maxsize=None)
def binary_image(B, h, w):
    """[B, 3, h, w] float32 of 0 and 1024: steps along rows and columns (half planes toggled), rectangles and single pixels, each in
    one channel or in all three.  The first seed whose image passes binary_image_report is taken (tiny maps need a few)."""
    for attempt in range(512):
        g = _gen("binary-image", B, h, w, attempt)
        r = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
        on = torch.zeros(B, 3, h, w, dtype=torch.bool)
        for b in range(B):
            kinds = ["pixel"] * (1 + h * w // 64) + ["box"] * (1 + h * w // 256)
            if h * w > 16:
                kinds += ["row"] * (1 + h // 16) + ["col"] * (1 + w // 32)
            for kind in kinds:
                c = r(0, 4)                                   # one channel (three in five) or all three
                ch = slice(c, c + 1) if c < 3 else slice(0, 3)
                y0, x0 = r(0, h - 1), r(0, w - 1)
                y1, x1 = {"pixel": (y0 + 1, x0 + 1), "box": (r(y0 + 1, h), r(x0 + 1, w)), "row": (h, w), "col": (h, w)}[kind]
                if kind == "row":
                    x0 = 0
                if kind == "col":
                    y0 = 0
                on[b, ch, y0:y1, x0:x1] ^= True
        img = on.float() * STEP
        if _report_ok(binary_image_report(img)):
            return img
    raise AssertionError("no binary image for %s" % ((B, h, w),))


def dyadic_image(B, h, w):
    """[B, 3, h, w] float32 multiples of 2^-8 in [0, 0.5]: every |second difference| <= 1, so |arg| <= 1 for a <= 1."""
    return torch.randint(0, 129, (B, 3, h, w), generator=_gen("dyadic-image", B, h, w)).float() * IMG_UNIT


# ---- smoothness ------------------------------------------------------------------------------------------------------------------------------

def mean_inv_f32(disp):
    """The kernels' per-sample mean (an exact sum, one correctly rounded float32 division) and inv = 1.f / (mean + 1e-7f), in float32."""
    B, h, w = disp.shape
    check_exact(DISP_UNIT, [disp], [disp.abs().sum((1, 2))])
    mean = disp.sum((1, 2)).float() / torch.tensor(float(h * w), dtype=torch.float32)
    return mean, torch.tensor(1.0, dtype=torch.float32) / (mean + torch.tensor(1e-7, dtype=torch.float32))


def smooth_core(disp, w6, inv, normalize, weight, gw):
    """The operation itself in float64: disp [B, h, w], weights w6 [6, B, h, w] (0 outside the domains), inv [B] (ones without
    normalisation), gw = upstream gradient x weight.  Per term and anchor t_k and |t_k| w_k, the loss, the gradient g with respect to
    disp inv, sum |addend| of g, and d_disp through the adjoint of disp / (mean + eps): g inv - (sum g disp) inv^2 / (h w)."""
    B, h, w = disp.shape
    cnt = counts(B, h, w)
    raw = six_terms(disp)
    t = raw * inv[None, :, None, None]
    fwd = t.abs() * w6
    loss = weight * sum(float(fwd[k].sum()) / cnt[k] for k in range(6))
    S = torch.sign(t) * w6 * torch.tensor([gw / c for c in cnt], dtype=F64)[:, None, None, None]
    g, T = six_adjoint(S), six_adjoint(S, magnitudes=True)
    d = g
    if normalize:
        d = g * inv[:, None, None] - ((g * disp).sum((1, 2)) * inv * inv / float(h * w))[:, None, None]
    return types.SimpleNamespace(raw=raw, t=t, fwd=fwd, loss=loss, g=g, T=T, d=d)


@functools.lru_cache(maxsize=4)
def smooth_case(B, h, w, mode):
    """mode "zero": normalize = 0, zero-rich disparity, binary weights (everything exact).  "nozero": normalize = 1, no-zero
    disparity, binary weights.  "nozero-dyadic": normalize = 1, a dyadic image in [0, 0.5].  All references float64; with
    normalize = 1 they are evaluated with the kernel's own float inv."""
    normalize = mode != "zero"
    disp = (nozero_disp if normalize else zero_rich_disp)(B, h, w)
    img = dyadic_image(B, h, w) if mode == "nozero-dyadic" else binary_image(B, h, w)
    wrel = W_REL if mode == "nozero-dyadic" else 0
    w6 = exp_weights(img, 0.5) if wrel else binary_weights(img)
    mean, inv32 = mean_inv_f32(disp)
    inv = inv32.double() if normalize else torch.ones(B, dtype=F64)
    weight = SMOOTH_WEIGHT
    cnt = counts(B, h, w)
    core = smooth_core(disp, w6, inv, normalize, weight, SMOOTH_GSCALE * weight)
    raw, t, fwd, loss, g, T = core.raw, core.t, core.fwd, core.loss, core.g, core.T
    partial = torch.stack([tile_sums(fwd[k]) for k in range(6)], 1)              # [blocks, 6]
    if not normalize:
        check_exact(DISP_UNIT, [raw], [fwd[k].sum() for k in range(6)])
    e_g = gamma(G_C + (wrel + 1 if wrel else 0)) * T
    out = types.SimpleNamespace(B=B, h=h, w=w, normalize=int(normalize), disp=disp, img=img, w6=w6, mean=mean, inv=inv, raw=raw, t=t,
                                partial=partial, loss=loss, g=g, T=T, e_g=e_g, wrel=wrel, nblk=smooth_num_blocks(B, h, w))
    if not normalize:
        out.e_partial, out.e_loss = torch.zeros_like(partial), gamma(7) * loss
        out.d, out.e_d = g, e_g
        return out
    M = (disp * inv[:, None, None]).abs().amax((1, 2))                             # [B]
    e_t = TERM_ROUNDINGS * U * (1.0 + U) * M[None, :, None, None] * w6             # per anchor and term
    gp = gamma(13 + wrel)
    out.e_partial = torch.stack([(1 + gp) * tile_sums(e_t[k]) + gp * tile_sums(fwd[k]) for k in range(6)], 1)
    out.e_loss = weight * sum(float((1 + gamma(15)) * out.e_partial[:, k].sum() + gamma(15) * partial[:, k].sum()) / cnt[k]
                              for k in range(6))
    out.dot = tile_sums(g * disp)
    out.e_dot = (1 + gamma(13)) * tile_sums(disp.abs() * e_g) + gamma(13) * tile_sums((g * disp).abs())
    per = out.nblk // B
    n = float(h * w)
    corr = out.dot.reshape(B, per).sum(1) * inv * inv / n
    e_corr = ((1 + gamma(11)) * out.e_dot.reshape(B, per).sum(1) + gamma(11) * out.dot.abs().reshape(B, per).sum(1)) * inv * inv / n
    out.d = g * inv[:, None, None] - corr[:, None, None]
    out.e_d = ((1 + gamma(2)) * (e_g * inv[:, None, None] + e_corr[:, None, None])
               + gamma(2) * ((g * inv[:, None, None]).abs() + corr.abs()[:, None, None]))
    return out


# ---- feature regulariser ---------------------------------------------------------------------------------------------------------------------

WT_BASE = (0, 2, 4, 7, 11, 15)           # codes: dx 2, dy 2, dxx 3, dxy 4, dyx 4, dyy 3 -- 18 in all
GATHERS = tuple((k, ay, ax) for k, offs in enumerate((((0, 0), (0, -1)), ((0, 0), (-1, 0)), ((0, 0), (0, -1), (0, -2)),
                                                      ((0, 0), (0, -1), (-1, 0), (-1, -1)), ((0, 0), (0, -1), (-1, 0), (-1, -1)),
                                                      ((0, 0), (-1, 0), (-2, 0)))) for ay, ax in offs)


def fabricate_wt(B, h, w):
    """Caller-made weights [B, 6, h, w] float64: magnitudes 0.25 (1 + code), code = (base_k + position class + 5 b) mod 18, where the
    position class (x mod 2, y mod 2, x mod 3, (y mod 2, x mod 2), the same, y mod 3) separates the anchors of one term that touch
    one pixel; the first two terms negative; 0 outside each term's domain."""
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    pos = (x % 2, y % 2, x % 3, 2 * (y % 2) + x % 2, 2 * (y % 2) + x % 2, y % 3)
    b = torch.arange(B)[:, None, None, None]
    code = (torch.stack([WT_BASE[k] + pos[k] for k in range(6)])[None] + 5 * b) % 18
    sign = torch.tensor([-1.0, -1.0, 1.0, 1.0, 1.0, 1.0], dtype=F64)[None, :, None, None]
    return sign * 0.25 * (code.double() + 1.0) * domains(h, w)[None]


def gathered_weights(Wt):
    """[18, B, h, w]: the weight of GATHERS[j] = (term, dy, dx) as seen from each pixel, NaN where that anchor does not exist."""
    B, _, h, w = Wt.shape
    dom = domains(h, w)
    out = torch.full((len(GATHERS), B, h, w), NAN, dtype=F64)
    for j, (k, ay, ax) in enumerate(GATHERS):
        src = torch.where(dom[k][None], Wt[:, k], torch.full_like(Wt[:, k], NAN))
        out[j, :, -ay:, -ax:] = src[:, :h + ay, :w + ax]
    return out


def featreg_refs(feat, Wt, gscale):
    """feat [B, C, h, w], Wt [B, 6, h, w] float64 -> per pixel and channel: the forward addend sum_k |t_k| Wt_k, its magnitude sum, the
    gradient gscale sum (anchor, term) sign(t_k) Wt_k stencil entry, and the magnitude sum of that."""
    t = six_terms(feat)                                          # [6, B, C, h, w]
    W = Wt.permute(1, 0, 2, 3)[:, :, None]                       # [6, B, 1, h, w]
    fwd = (t.abs() * W).sum(0)
    S = torch.sign(t) * W
    return fwd, (t.abs() * W.abs()).sum(0), gscale * six_adjoint(S), gscale * six_adjoint(S, magnitudes=True)


@functools.lru_cache(maxsize=None)
def featreg_case(B, C, h, w):
    """Integer features in [-32, 32] with caller-made dyadic weights (exact), and the same features under the binary-weight image with
    the host's float scales coef_k / count_k (bounded)."""
    g = _gen("featreg", B, C, h, w)
    feat = torch.randint(-32, 33, (B, C, h, w), generator=g).double()
    assert torch.equal(bf(feat).double(), feat)
    Wt = fabricate_wt(B, h, w)
    fwd, mag, grad, _ = featreg_refs(feat, Wt, FEATREG_GSCALE)
    check_exact(0.25, [Wt, fwd], [featreg_block_sums(mag)])
    check_exact(0.125, [grad])
    dis, cvt = 1e-3, 2e-3
    img = binary_image(B, h, w)
    scale = [f32(c / k) for c, k in zip((-dis, -dis, cvt, cvt, cvt, cvt), counts(B * C, h, w))]
    Wt2 = edge_weights_ref(binary_weights(img), scale)
    fwd2, mag2, grad2, gmag2 = featreg_refs(feat, Wt2, FEATREG_GSCALE)
    return types.SimpleNamespace(B=B, C=C, h=h, w=w, feat=feat, Wt=Wt, partial=featreg_block_sums(fwd), grad=grad, dis=dis, cvt=cvt,
                                 img=img, loss2=float(fwd2.sum()), e_loss2=gamma(32) * float(mag2.sum()), grad2=grad2,
                                 e_grad2=gamma(18) * gmag2, nblk=featreg_num_blocks(B, h, w, C))


# ---- area mean, td_sum_scaled ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def area_case(fy, fx, B, C, h, w):
    """A multiple-of-2^-8 image [B, C, h fy, w fx] and its area mean: the exact window sum as float32, divided ONCE in float32."""
    img = torch.randint(0, 256, (B, C, h * fy, w * fx), generator=_gen("area", fy, fx, B, C, h, w)).double() * IMG_UNIT
    sums = img.reshape(B, C, h, fy, w, fx).sum((3, 5))
    check_exact(IMG_UNIT, [img], [sums])
    n = fy * fx
    G = area_group(n)
    return types.SimpleNamespace(img=img.float(), out=sums.float() / torch.tensor(float(n), dtype=torch.float32), n=n, G=G,
                                 ragged=n % G != 0, blocks=area_blocks(B * C * h * w, G))


def sum_scaled_case(n):
    p = 0.25 * torch.randint(-32, 33, (n,), generator=_gen("sum-scaled", n)).double()
    check_exact(0.25, [p], [p.abs().sum()])
    return p.float(), torch.tensor([float(p.sum()) * 0.5], dtype=torch.float32)


# ---- masked reconstruction ---------------------------------------------------------------------------------------------------------------------

SSIM_C1, SSIM_C2, L1_EPS2 = 0.01 ** 2, 0.03 ** 2, 1e-6


def _box3_reflect(v):
    """The mean over the 3 x 3 window under ReflectionPad(1), by explicit index lists and nine slices."""
    h, w = v.shape[-2:]
    p = v[..., [1] + list(range(h)) + [h - 2], :][..., :, [1] + list(range(w)) + [w - 2]]
    return sum(p[..., dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0


def recon_ref(x, y, hole):
    """S = sum_p hole(p) (0.85 mean_c SSIM_c + 0.15 mean_c sqrt((y - x)^2 + 1e-6)) and dS/dx in float64; x, y [B, 3, h, w], hole
    [B, h, w]."""
    x = x.double().clone().requires_grad_(True)
    y = y.double()
    mx, my = _box3_reflect(x), _box3_reflect(y)
    vx, vy, cxy = _box3_reflect(x * x) - mx * mx, _box3_reflect(y * y) - my * my, _box3_reflect(x * y) - mx * my
    ssim = (2 * mx * my + SSIM_C1) * (2 * cxy + SSIM_C2) / ((mx * mx + my * my + SSIM_C1) * (vx + vy + SSIM_C2))
    per = 0.85 * torch.clamp((1 - ssim) / 2, 0, 1).mean(1) + 0.15 * torch.sqrt((y - x) ** 2 + L1_EPS2).mean(1)
    S = (per * hole.double()).sum()
    S.backward()
    return float(S.detach()), x.grad


@functools.lru_cache(maxsize=None)
def recon_case(B, h, w):
    """Smooth frames as in tests/test_hip_recon.py, a hole weight in {0 .. 3} that is at least 1 on all four borders."""
    from tests.util import smooth_image
    g = _gen("recon", B, h, w)
    x = smooth_image(g, B, 3, max(h, 8), max(w, 8))[:, :, :h, :w].contiguous()
    y = (x + 0.08 * torch.randn(B, 3, h, w, generator=g)).clamp(0, 1)
    hole = torch.randint(0, 4, (B, h, w), generator=g).float()
    ring = torch.ones(h, w, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    hole = torch.where(ring[None], hole.clamp(min=1.0), hole)
    S, grad = recon_ref(x, y, hole)
    return types.SimpleNamespace(B=B, h=h, w=w, x=x, y=y, hole=hole, S=S, grad=0.5 * grad, fwd=recon_geometry(B, h, w, RC_FWD_COLS),
                                 bwd=recon_geometry(B, h, w, RC_BWD_COLS))


# ---- fenced device buffers -----------------------------------------------------------------------------------------------------------------------
Out = collections.namedtuple("Out", "t fence")


def guard(t, dtype=None):
    """The host tensor `t` (any shape, dense) on the device between NaN guard rows: a read past either end poisons the result."""
    t = t.to(dtype or t.dtype).contiguous()
    return fenced_input(t.reshape(-1, t.shape[-1])).view(t.shape)


def guard_out(shape, dtype=torch.float32, init=None):
    """An output of `shape`: NaN inside (or `init`, for a buffer that is accumulated into), marker guard rows around it."""
    cols = shape[-1]
    f = fenced_output(int(torch.tensor(shape).prod()) // cols, cols, dtype)
    if init is not None:
        f.view.copy_(init.reshape(f.view.shape))
    return Out(f.view.view(tuple(shape)), f)


def assert_guard(o, what=""):
    """Every element was written (no NaN left) and no guard row was touched."""
    assert_fence(o.fence, what)
