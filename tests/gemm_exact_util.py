"""Exact tests of the MFMA GEMM kernel family (csrc/td_conv1x1.hip, td_conv3x3.hip, td_conv3x3_wgrad.hip, td_conv_tile.h): the case
tables, integer operands, float64 references and the fenced device buffers that tests/test_gemm_exact_cpu.py (no GPU) and
tests/test_hip_gemm_exact.py share.

The idea: with small INTEGER operands (activations, gradients and residuals in [-3, 3], weights in {-1, 0, 1}; BatchNorm parameters
that are small powers of two) every product and every partial sum these kernels form is a multiple of one power of two u and stays
below 2^24 u in magnitude, so the fp32 accumulation is exact in ANY order: the stored result must equal the float64 reference,
rounded to bf16 exactly where the kernel rounds, bit for bit -- and so must the epilogue statistics.  No tolerance, hence no room for
a kernel that is nearly right (a few rows of a ragged tile counted twice, a stage of the deep pipeline skipped).  check_exact states
that precondition on the reference alone; a case that violates it has the wrong inputs.

Every builder is deterministic (seeded by its own arguments) and cached: the tests of one shape share one reference."""
import collections
import functools
import types
import zlib

import torch
import torch.nn.functional as F

BF = torch.bfloat16
NAN = float("nan")
LIMIT = 2.0 ** 24          # integers up to here are fp32 values, and so is every sum of them whose terms' magnitudes add up to less

# ---- the case tables -------------------------------------------------------------------------------------------------------------
# Row cases of the forward / data-gradient GEMMs: Mg rows per statistics group, G groups, `width` output columns; (bm, bn) is the
# tile cv_pick_tile chooses for it and `last` the number of valid rows in a group's last tile.
RowCase = collections.namedtuple("RowCase", "id Mg G width bm bn last")
ROW_CASES = (
    RowCase("r1", 1, 1, 64, 64, 64, 1),
    RowCase("r2", 65, 1, 64, 64, 64, 1),
    RowCase("r3", 129, 3, 128, 64, 64, 1),          # groups start at rows 129 and 258: inside a tile's span in memory
    RowCase("r4", 14241, 1, 256, 128, 64, 33),      # crosses the `lr + 32 < rows_valid` store of a_side
    RowCase("r5", 7105, 1, 1024, 128, 128, 65),
    RowCase("r6", 3457, 2, 1024, 128, 128, 1),      # second group unaligned
    RowCase("r7", 897, 64, 64, 128, 64, 1),         # the largest group count the entry points accept
)
ROWS = {rc.id: rc for rc in ROW_CASES}
# reduction widths: 64 one stage; 128 two stages, not deep; 192 three stages (the smallest and an odd deep pipeline); 320 five
REDUCTIONS = {"r1": (64, 128, 192, 320), "r2": (64, 128, 192, 320), "r3": (64, 128, 192, 320), "r4": (64, 128, 192, 320),
              "r5": (64, 192), "r6": (64, 192), "r7": (64, 128, 192, 320)}      # 128 x 128 tiles are never deep
GEMM_COMBOS = tuple((rc.id, red) for rc in ROW_CASES for red in REDUCTIONS[rc.id])
IN_ROWS = (1, 16, 17, 33)   # partial rows handed to a fused prologue: no shrink, the limit, two in-place shrinks (stride 2 and 3)

# td_conv1x1_fwd with stride 2: (B, Hi, Wi, groups), K = 64 -> N in (64, 128)
STRIDE2_CASES = ((2, 5, 7, 1), (3, 6, 8, 3), (1, 1, 1, 1))

# td_conv1x1_wgrad: (M, K, N, B, Hi, Wi, stride, P, stages per launched row range)
WgradCase = collections.namedtuple("WgradCase", "M K N B Hi Wi stride P stages")
WGRAD_CASES = (
    WgradCase(1, 64, 64, 1, 1, 1, 1, 1, (1,)),
    WgradCase(64, 64, 64, 1, 1, 64, 1, 1, (1,)),
    WgradCase(65, 64, 128, 1, 1, 65, 1, 1, (2,)),
    WgradCase(129, 128, 64, 1, 1, 129, 1, 1, (3,)),
    WgradCase(257, 64, 64, 1, 1, 257, 1, 2, (3, 2)),
    WgradCase(321, 64, 64, 1, 1, 321, 1, 2, (3, 3)),
    WgradCase(3073, 512, 512, 1, 1, 3073, 1, 12, (5,) * 9 + (4,)),     # P = 12, ten ranges launched: two trailing slabs never written
    WgradCase(24, 64, 64, 2, 5, 7, 2, 1, (1,)),                        # stride 2: 3 x 4 of the 5 x 7 pixels of each image
)

# td_conv3x3_fwd: (B, Hi, Wi, Cin, N, stride, pad, groups, bm, bn)
Conv3Case = collections.namedtuple("Conv3Case", "B Hi Wi Cin N stride pad groups bm bn")
CONV3_CASES = (
    Conv3Case(1, 3, 3, 8, 64, 1, 0, 1, 64, 64),             # one output pixel, an 8-channel chunk
    Conv3Case(2, 5, 7, 72, 64, 1, 1, 1, 64, 64),            # a second chunk of 8 channels; 70 rows: ragged, crosses the image boundary
    Conv3Case(3, 6, 9, 64, 128, 2, 1, 3, 64, 64),           # stride 2, 15 rows per group
    Conv3Case(2, 4, 6, 8, 64, 2, 0, 1, 64, 64),             # stride 2 without padding, Ho = 1
    Conv3Case(13, 1, 1093, 8, 256, 1, 1, 1, 128, 64),       # 14209 rows, every row has padding above and below
    Conv3Case(3, 3, 2349, 8, 1024, 1, 0, 1, 128, 128),      # 7041 rows, 1 valid row in the last tile
)

# td_conv3x3_wgrad: (B, Ho, Wo, C, N, P, stages per launched row range); each with pad 0 and pad 1
W3Case = collections.namedtuple("W3Case", "B Ho Wo C N P stages")
W3_CASES = (
    W3Case(1, 4, 20, 64, 64, 1, (2,)),                      # the gate's minimum, 80 pixels
    W3Case(1, 4, 21, 64, 64, 1, (2,)),
    W3Case(2, 4, 20, 64, 128, 1, (3,)),                     # the image boundary (pixel 80) falls inside stage 1
    W3Case(1, 5, 52, 128, 64, 2, (3, 2)),                   # 260 pixels
)


def pick_tile(Mg, G, N):
    """Replica of cv_pick_tile in csrc/td_conv_tile.h (a change there must be made here too: the case tables rest on it)."""
    blocks = lambda bm, bn: G * (-(-Mg // bm)) * (N // bn)
    if N % 128 == 0 and blocks(128, 128) >= 448:
        return 128, 128
    return (128, 64) if blocks(128, 64) >= 448 else (64, 64)


def dispatched(rc, red, prologue=0):
    """(bm, bn, deep) as cv_dispatch in csrc/td_conv1x1.hip instantiates it: prologue 2 (td_conv1x1_dgrad_bnbwd) demotes 128 x 128 to
    128 x 64; the two-register-set pipeline runs from three K stages on 64 x 64 tiles and on 128 x 64 ones without a prologue."""
    bm, bn = pick_tile(rc.Mg, rc.G, rc.width)
    if prologue == 2 and (bm, bn) == (128, 128):
        bn = 64
    deep = red >= 192 and ((bm, bn) == (64, 64) or ((bm, bn) == (128, 64) and prologue == 0))
    return bm, bn, deep


def split_ranges(M, tiles, target):
    """Replica of wg_splits (csrc/td_conv1x1.hip, target 768) / w3_splits (csrc/td_conv3x3_wgrad.hip, target 256) and of the row ranges
    the entry points cut: (P, stages of 64 rows per LAUNCHED range) -- trailing empty ranges are not launched."""
    P = max(1, min(-(-target // tiles), -(-M // 256), 512))
    rps = -(-(-(-M // P)) // 64) * 64
    return P, tuple(-(-(min(M, lo + rps) - lo) // 64) for lo in range(0, M, rps))


# ---- the exactness precondition ----------------------------------------------------------------------------------------------------

def check_exact(unit, values=(), abs_sums=()):
    """Every element of `values` is a multiple of the power of two `unit`, and every entry of `abs_sums` -- the sum of |terms| of a
    sum the kernel forms, or an upper bound of it -- is below 2^24 unit: then each partial sum, in any order, is an fp32 value."""
    assert unit > 0 and float(torch.tensor(unit).log2()) % 1 == 0
    for v in values:
        q = v.double() / unit
        assert bool(torch.isfinite(q).all()) and torch.equal(q, q.round()), "not multiples of %g" % unit
    for s in abs_sums:
        top = float(s.max()) if isinstance(s, torch.Tensor) else float(s)
        assert top < LIMIT * unit, (top, LIMIT * unit)


def tile_sums(v, G, Mg, bm):
    """[G * Mg, N] float64 -> [G, ceil(Mg / bm), N]: column sums over the rows of each row tile of each group."""
    N = v.shape[1]
    S = -(-Mg // bm)
    p = torch.zeros(G, S * bm, N, dtype=torch.float64)
    p[:, :Mg] = v.reshape(G, Mg, N)
    return p.reshape(G, S, bm, N).sum(2)


def one_ulp(got, ref):
    """got is ref or one of its two float32 neighbours, element by element."""
    inf = torch.full_like(ref, float("inf"))
    return bool(((got == ref) | (got == torch.nextafter(ref, inf)) | (got == torch.nextafter(ref, -inf))).all())


# ---- operand generators ------------------------------------------------------------------------------------------------------------

def _gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def ints(g, shape, lo, hi):
    """Uniform integers in [lo, hi] as bf16 (exact).  Random draws: asymmetric, a transposed or permuted operand map cannot pass."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int8).to(BF)


def acts(g, shape):
    return ints(g, shape, -3, 3)


def weights(g, shape):
    return ints(g, shape, -1, 1)


def pick(g, shape, choices):
    """Uniform draws from `choices` as float32."""
    return torch.tensor(choices, dtype=torch.float32)[torch.randint(0, len(choices), tuple(shape), generator=g)]


def bf(v):
    """One round-to-nearest-even to bf16 of a float64 (or float32) tensor of values that float32 holds exactly."""
    return v.float().to(BF)


def fabricate_partials(g, G, R, K, A, B):
    """[G, R, K, 2] float32 partial rows, multiples of 0.5, that sum over R to (A[g], B[g]) for every channel of group g."""
    p = 0.5 * torch.randint(-8, 9, (G, R, K, 2), generator=g).double()
    p[:, 0] = 0
    tgt = torch.stack([torch.as_tensor(A, dtype=torch.float64), torch.as_tensor(B, dtype=torch.float64)], -1)[:, None, :]
    p[:, 0] = tgt - p.sum(1)
    check_exact(0.5, [p], [p.abs().sum(1)])
    assert torch.equal(p.sum(1), tgt.expand(G, K, 2))
    return p.float()


def in_rows_for(rid, red, shift=0):
    return IN_ROWS[(GEMM_COMBOS.index((rid, red)) + shift) % len(IN_ROWS)]


# ---- references: 1x1 GEMMs ---------------------------------------------------------------------------------------------------------

def _stat_reference(y, rc, bm, second=None, unit=1.0):
    """Per-tile (sum y, sum y * second) of the stored values (second: y itself), with the precondition for those sums."""
    yd = y.double()
    sd = yd if second is None else second
    check_exact(unit, [yd], [tile_sums(yd.abs(), rc.G, rc.Mg, bm)])
    check_exact(unit * unit if second is None else unit, [yd * sd], [tile_sums((yd * sd).abs(), rc.G, rc.Mg, bm)])
    return torch.stack([tile_sums(yd, rc.G, rc.Mg, bm), tile_sums(yd * sd, rc.G, rc.Mg, bm)], -1)      # [G, S, N, 2]


@functools.lru_cache(maxsize=2)
def forward_case(rid, red):
    """td_conv1x1_fwd / td_conv1x1_fwd_sum: y = bf(X W^T), per-tile statistics of the stored y, run_out = bf(float(y) + run_in)."""
    rc = ROWS[rid]
    M, g = rc.Mg * rc.G, _gen("fwd", rid, red)
    x, w = acts(g, (M, red)), weights(g, (rc.width, red))
    check_exact(1.0, [x, w], [red * 3.0])
    y = bf(x.double() @ w.double().t())
    run_in = acts(g, (M, rc.width))
    run_out = bf(y.double() + run_in.double())
    return types.SimpleNamespace(rc=rc, M=M, x=x, w=w, y=y, stats=_stat_reference(y, rc, rc.bm), run_in=run_in, run_out=run_out)


@functools.lru_cache(maxsize=None)
def stride2_case(B, Hi, Wi, groups, N):
    g = _gen("stride2", B, Hi, Wi, groups, N)
    K, Ho, Wo = 64, (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    x, w = acts(g, (B, Hi, Wi, K)), weights(g, (N, K))
    rc = RowCase("s2", B * Ho * Wo // groups, groups, N, 64, 64, None)
    y = bf(x[:, ::2, ::2].reshape(-1, K).double() @ w.double().t())
    return types.SimpleNamespace(rc=rc, M=B * Ho * Wo, x=x.reshape(-1, K), w=w, y=y, stats=_stat_reference(y, rc, 64))


def _bn_params(g, G, C):
    """Dyadic BatchNorm parameters: gamma in {1, 2}, beta a multiple of 0.5, an integer mean and invstd in {1, 0.5} per group and channel."""
    gamma, beta = pick(g, (C,), (1.0, 2.0)), 0.5 * torch.randint(-4, 5, (C,), generator=g).float()
    mean, invstd = torch.randint(-2, 3, (G, C), generator=g).float(), pick(g, (G, C), (1.0, 0.5))
    return gamma, beta, mean, invstd


def _relu_mask(z, rc, gamma, beta, mean, invstd):
    """[bn(z) > 0] as the kernels recompute it: fma(z, gamma invstd, beta - mean gamma invstd) > 0, exact in multiples of 0.5; the
    case must hold elements that are exactly 0 (masked)."""
    sc = (gamma * invstd).double()                                     # [G, C]
    sh = beta.double() - mean.double() * sc
    pre = z.double().reshape(rc.G, rc.Mg, -1) * sc[:, None] + sh[:, None]
    check_exact(0.5, [pre])
    assert bool((pre == 0).any()) and bool((pre > 0).any()) and bool((pre < 0).any())
    return (pre > 0).reshape(z.shape).double()


@functools.lru_cache(maxsize=2)
def dgrad_case(rid, red):
    """td_conv1x1_dgrad [+ residual] and td_conv1x1_dgrad_bnsums: dx = bf(dY W), W [Cout = red, Cin = width] as the forward stores it."""
    rc = ROWS[rid]
    M, g = rc.Mg * rc.G, _gen("dgrad", rid, red)
    dy, w = acts(g, (M, red)), weights(g, (red, rc.width))
    check_exact(1.0, [dy, w], [red * 3.0])
    dx = bf(dy.double() @ w.double())
    res = acts(g, (M, rc.width))
    dx_res = bf(dx.double() + res.double())
    z = acts(g, (M, rc.width))
    gamma, beta, mean, invstd = _bn_params(g, rc.G, rc.width)
    gm = dx.double() * _relu_mask(z, rc, gamma, beta, mean, invstd)
    zc = (z.double().reshape(rc.G, rc.Mg, -1) - mean.double()[:, None]).reshape(M, -1)
    return types.SimpleNamespace(rc=rc, M=M, dy=dy, w=w, dx=dx, res=res, dx_res=dx_res, z=z, gamma=gamma, beta=beta, mean=mean,
                                 invstd=invstd, sums=_stat_reference(gm, rc, rc.bm, second=zc))


@functools.lru_cache(maxsize=2)
def bnrelu_case(rid, red, in_rows, momentum=0.25):
    """td_conv1x1_fwd_bnrelu: the statistics come from in_partials alone, so they are fabricated: group g has mean m_g = 2 + g,
    variance 0.5 and eps = 0.5, i.e. (in double, every operation correctly rounded) save_mean == m_g and save_invstd == 1.  z lies
    around its group's mean (m_g + [-3, 3]); with integer gamma and beta the staged operand a = relu((z - m_g) gamma + beta) is an
    exact integer, a_side == a and y == bf(a W^T)."""
    rc = ROWS[rid]
    M, K, g = rc.Mg * rc.G, red, _gen("bnrelu", rid, red, in_rows)
    m = torch.arange(rc.G, dtype=torch.float64) + 2
    z = bf(acts(g, (rc.G, rc.Mg, K)).double() + m[:, None, None]).reshape(M, K)
    w = weights(g, (rc.width, K))
    gamma, beta = pick(g, (K,), (1.0, 2.0)), torch.randint(-2, 3, (K,), generator=g).float()
    part = fabricate_partials(g, rc.G, in_rows, K, m * rc.Mg, (m * m + 0.5) * rc.Mg)
    sh = beta.double()[None] - m[:, None] * gamma.double()[None]                      # [G, K]: beta - mean * gamma * invstd
    pre = z.double().reshape(rc.G, rc.Mg, K) * gamma.double() + sh[:, None]
    check_exact(1.0, [z, w, pre, sh], [pre.abs().max() + sh.abs().max()])
    a = bf(pre.clamp(min=0).reshape(M, K))
    assert bool((a == 0).any()) and bool((a > 0).any())
    check_exact(1.0, [a], [K * float(a.max())])
    y = bf(a.double() @ w.double().t())
    rm0, rv0 = torch.randint(-2, 3, (K,), generator=g).float(), pick(g, (K,), (1.0, 0.5, 2.0))
    rm, rv = rm0.double(), rv0.double()
    for grp in range(rc.G):       # one momentum update per group, in order; each rounded to float as the kernel does
        unbiased = 0.5 * (rc.Mg / (rc.Mg - 1)) if rc.Mg > 1 else 0.5
        rm = ((1.0 - momentum) * rm + momentum * float(m[grp])).float().double()
        rv = ((1.0 - momentum) * rv + momentum * unbiased).float().double()
    return types.SimpleNamespace(rc=rc, M=M, z=z, w=w, gamma=gamma, beta=beta, part=part, in_rows=in_rows, eps=0.5, momentum=momentum,
                                 mean=m.float()[:, None].expand(rc.G, K).contiguous(), a=a, y=y, stats=_stat_reference(y, rc, rc.bm),
                                 rm0=rm0, rv0=rv0, rm=rm.float(), rv=rv.float())


@functools.lru_cache(maxsize=2)
def bnbwd_case(rid, red, in_rows):
    """td_conv1x1_dgrad_bnbwd with backward sums that are zero (1 / Mg is not exact for a ragged Mg): dz = bf(gamma invstd g [bn(z) > 0]),
    dz_side == dz, dx = bf(dz W) [+ residual], dgamma == dbeta == 0."""
    rc = ROWS[rid]
    M, g = rc.Mg * rc.G, _gen("bnbwd", rid, red, in_rows)
    gr, z, w = acts(g, (M, red)), acts(g, (M, red)), weights(g, (red, rc.width))
    rcz = rc._replace(width=red)
    gamma, beta, mean, invstd = _bn_params(g, rc.G, red)
    c0 = (gamma * invstd).double()                                     # [G, red]
    dzd = (gr.double() * _relu_mask(z, rcz, gamma, beta, mean, invstd)).reshape(rc.G, rc.Mg, red) * c0[:, None]
    dz = bf(dzd.reshape(M, red))
    check_exact(0.5, [dzd, dz, w], [red * 6.0])                        # |dz| <= 2 * 3, |w| <= 1
    assert torch.equal(dz.double(), dzd.reshape(M, red))
    dx = bf(dz.double() @ w.double())
    res = acts(g, (M, rc.width))
    return types.SimpleNamespace(rc=rc, M=M, g=gr, z=z, w=w, gamma=gamma, beta=beta, mean=mean, invstd=invstd, in_rows=in_rows,
                                 part=torch.zeros(rc.G, in_rows, red, 2), dz=dz, dx=dx, res=res, dx_res=bf(dx.double() + res.double()))


# ---- references: weight gradients and the 3x3 kernels ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def wgrad_case(i):
    """td_conv1x1_wgrad: dW [N, K] = dY^T X over the M output pixels (stride 2: the pixels x[:, ::2, ::2])."""
    c = WGRAD_CASES[i]
    g = _gen("wgrad", i)
    x = acts(g, (c.B, c.Hi, c.Wi, c.K))
    xs = x[:, ::c.stride, ::c.stride].reshape(-1, c.K)
    assert xs.shape[0] == c.M
    dy = acts(g, (c.M, c.N))
    check_exact(1.0, [x, dy], [c.M * 9.0])
    dw = dy.double().t() @ xs.double()
    return types.SimpleNamespace(c=c, x=x.reshape(-1, c.K), dy=dy, dw=dw)


@functools.lru_cache(maxsize=None)
def conv3_case(i):
    """td_conv3x3_fwd: y = bf(conv2d(x, w)) in float64; x is kept [B, Hi, Wi, Cin], w [N, 3, 3, Cin] (channels-last memory)."""
    c = CONV3_CASES[i]
    g = _gen("conv3", i)
    x, w = acts(g, (c.B, c.Hi, c.Wi, c.Cin)), weights(g, (c.N, 3, 3, c.Cin))
    check_exact(1.0, [x, w], [9 * c.Cin * 3.0])
    yd = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), stride=c.stride, padding=c.pad)
    B, N, Ho, Wo = yd.shape
    assert (Ho, Wo) == ((c.Hi + 2 * c.pad - 3) // c.stride + 1, (c.Wi + 2 * c.pad - 3) // c.stride + 1)
    y = bf(yd.permute(0, 2, 3, 1).reshape(-1, N))
    M = B * Ho * Wo
    rc = RowCase("c3", M // c.groups, c.groups, N, c.bm, c.bn, None)
    return types.SimpleNamespace(c=c, rc=rc, M=M, Ho=Ho, Wo=Wo, x=x, w=w, y=y, stats=_stat_reference(y, rc, c.bm))


@functools.lru_cache(maxsize=None)
def w3_case(i, pad):
    """td_conv3x3_wgrad: the float64 autograd weight gradient of conv2d (stride 1), laid out [N, 3, 3, C] like the weight's memory."""
    c = W3_CASES[i]
    g = _gen("w3", i, pad)
    Hi, Wi = c.Ho + 2 - 2 * pad, c.Wo + 2 - 2 * pad
    x, dy = acts(g, (c.B, Hi, Wi, c.C)), acts(g, (c.B, c.Ho, c.Wo, c.N))
    check_exact(1.0, [x, dy], [c.B * c.Ho * c.Wo * 9.0])
    w = torch.zeros(c.N, c.C, 3, 3, dtype=torch.float64, requires_grad=True)
    (F.conv2d(x.double().permute(0, 3, 1, 2), w, padding=pad) * dy.double().permute(0, 3, 1, 2)).sum().backward()
    return types.SimpleNamespace(c=c, pad=pad, x=x, dy=dy, dw=w.grad.permute(0, 2, 3, 1).contiguous())


# ---- fenced device buffers ---------------------------------------------------------------------------------------------------------
GUARD_ROWS = 136            # at least 4 are asked for; a whole 128-row tile written past the end still lands inside the allocation
MARKER = -24576.0           # -3 * 2^13: a bf16 and float32 value that no case produces

Fenced = collections.namedtuple("Fenced", "view buf fill")


def fenced(rows, cols, dtype, fill, device="cuda"):
    """`rows` rows (NaN) inside a larger device buffer with GUARD_ROWS guard rows of `fill` on either side.  Inputs take NaN guards (a
    read past the end that reaches the arithmetic poisons the result), outputs stay NaN inside and take MARKER guards."""
    buf = torch.full((rows + 2 * GUARD_ROWS, cols), fill, dtype=dtype, device=device)
    view = buf[GUARD_ROWS:GUARD_ROWS + rows]
    view.fill_(NAN)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return Fenced(view, buf, fill)


def fenced_input(t, device="cuda"):
    """The rows of the 2-D host tensor `t` on the device between NaN guard rows."""
    f = fenced(t.shape[0], t.shape[1], t.dtype, NAN, device)
    f.view.copy_(t)
    return f.view


def fenced_output(rows, cols, dtype=BF, device="cuda"):
    return fenced(rows, cols, dtype, MARKER, device)


def assert_fence(f, what=""):
    """After the call: every element inside was written (no NaN left, none from an input fence) and the guards hold the marker."""
    rows = f.view.shape[0]
    assert not bool(torch.isnan(f.view).any()), "%s: NaN in the output" % what
    guards = torch.cat([f.buf[:GUARD_ROWS], f.buf[GUARD_ROWS + rows:]])
    assert torch.equal(guards, torch.full_like(guards, f.fill)), "%s: a guard row was overwritten" % what
