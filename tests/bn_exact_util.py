"""Exact tests of the row-reduction kernels (csrc/td_bn.hip, csrc/td_biasact.hip): the case tables, integer operands and float64
references that tests/test_bn_exact_cpu.py (no GPU) and tests/test_hip_bn_exact.py share.  The technique is the one of
tests/gemm_exact_util.py, whose check_exact, generators and fenced buffers are imported, not copied: with small INTEGER activations
and gradients every sum these kernels form (sum x, sum x^2, sum g, sum g (x - mean)) is an fp32 value in any order, so a row that is
dropped or counted twice at a split boundary changes a result that is otherwise known to the last bit.  Three tiers of assertion:

statistics  bit-exact for ANY integer data: the per-split partial rows, the [G, C, 2] sums of the synchronised form, dbeta (exact
            sums), and save_mean / save_invstd / the running statistics: the kernels form mean, var, 1 / sqrt(var + eps) and the
            momentum update in double from the exact sums and round ONCE to float; stats_replica does the same operations in the
            same order (the library is built with -ffp-contract=off, double division and square root are correctly rounded on
            both sides).  dgamma = sum_g B_g invstd_g is fp32 arithmetic on exact sums: one product for G = 1 (bit-exact), G
            products added in order otherwise (within one ulp per added group of the same ordered float32 sum).
dyadic      bit-exact OUTPUTS: per channel and group x takes m - 1 and m + 1 equally often (m an integer), so mean = m, var = 1 and
            with eps = 3 invstd = 0.5 exactly; gamma in {1, 2} and beta a multiple of 0.5 make every y, residual sum and ReLU
            decision a multiple of 0.5.  Backward: g is fixed up on the last rows so that sum g and sum g (x - m) vanish (dx =
            gamma invstd g exactly) or, for one power-of-two Mg, are multiples of Mg (k1, k2, dx multiples of 1 / 8).
bounded     general integer data at ragged, odd Mg, against the float64 formula evaluated with the replica's own FLOAT mean and
            invstd (so the statistics' rounding does not enter), within a DERIVED bound, u = 2^-24:
              y  = fma(x, sc, sh) [+ res],  sc = gamma invstd (exact: gamma is a power of two),  sh = beta - mean sc (2 roundings)
                   |y - ref| <= 5 u (|x sc| + |mean sc| + |beta| + |res|)
              dx = fma(k0, g, fma(k1, x, k2)),  k0 = gamma invstd (exact),  k1 = -k0 invstd (B invstd) (1 / M): 5 roundings,
                   k2 = -k0 A (1 / M) - k1 mean: 3 roundings on the first term, k1 mean exact (the backward data has an integer mean
                   that is 0 or a power of two: its column sums are fixed up to m Mg, which also keeps g (x - mean) an integer)
                   |dx - ref| <= 8 u T,  T = |k0 g| + |k1 x| + |k1 mean| + |k0 A / M|     (5 + the subtraction + the two fma)
            plus half a bf16 spacing of the reference for bf16 outputs.

The host-side cut functions of the two kernel files are REPLICATED here (bn_splits, bn_rows_per_split, bn_stat_splits, bn_shrink,
ba_blocks): the case tables rest on them, so a change in csrc/td_bn.hip or csrc/td_biasact.hip must be mirrored here; the GPU file
cross-checks them against td_bn_partial_rows, td_bn_workspace_floats and td_bias_act_workspace_floats for every case.

Every builder is deterministic (seeded by its own arguments) and cached.  Nothing here touches a GPU at import."""
import collections
import functools
import types

import torch

from tests.gemm_exact_util import (BF, GUARD_ROWS, MARKER, NAN, _gen, assert_fence, bf, check_exact, fabricate_partials,  # noqa: F401
                                   fenced, fenced_input, fenced_output, ints, one_ulp, pick, tile_sums)

U = 2.0 ** -24              # unit round-off of float32
EPS_DYADIC = 3.0            # var 1 + eps 3 = 4: invstd = 0.5
EPS = float(torch.tensor(1e-5, dtype=torch.float32))            # what the C ABI's `float eps` holds
MOMENTUM_TENTH = float(torch.tensor(0.1, dtype=torch.float32))
LEAKY = torch.tensor(0.01, dtype=torch.float32)                 # the kernels' 0.01f

# ---- replicas of the host-side cut functions ----------------------------------------------------------------------------------------
BN_RY, BN_UNROLL, BN_STAT_BLOCKS, BN_PRO_MAX_S, BN_FIN_PARTS = 32, 4, 512, 96, 16
TD_THREADS = 256


def _cdiv(a, b):
    return -(-a // b)


def bn_splits(M, C, target_blocks, cap):
    return max(1, min(_cdiv(target_blocks, C // 64), _cdiv(M, 64), cap))


def bn_rows_per_split(M, S):
    return _cdiv(_cdiv(M, S), BN_RY) * BN_RY


def bn_stat_splits(Mg, C):
    S = bn_splits(Mg, C, BN_STAT_BLOCKS, 512)
    if S > 16 and (C // 64) * 16 >= 128:
        return bn_splits(Mg, C, (C // 64) * 16, 16)
    return S


def bn_shrink(S, max_rows=BN_PRO_MAX_S):
    """(Sq, Q) of bn_shrink_partials_to: Q shrink blocks of Sq partial rows each (the last one may be short); (1, S): no shrink."""
    if S <= max_rows:
        return 1, S
    Sq = _cdiv(S, max_rows)
    return Sq, _cdiv(S, Sq)


def bn_cut(Mg, C, stat=False):
    """How td_bn_fwd / td_bn_bwd (stat: td_bn_fwd_partials / td_bn_bwd_partials) cut a group of Mg rows: S splits asked for, rps rows per
    split, S_eff partial rows, the shrink (Sq, Q), the passes of the 4 x 32-row loop over a full split and the rows of the last split."""
    S = bn_stat_splits(Mg, C) if stat else bn_splits(Mg, C, BN_STAT_BLOCKS, 512)
    rps = bn_rows_per_split(Mg, S)
    S_eff = _cdiv(Mg, rps)
    Sq, Q = bn_shrink(S_eff)
    return types.SimpleNamespace(S=S, rps=rps, S_eff=S_eff, Sq=Sq, Q=Q, iters=_cdiv(rps, BN_RY * BN_UNROLL), last=Mg - (S_eff - 1) * rps)


def bn_workspace_floats(M, G, C):
    return (2 * bn_splits(M // G, C, BN_STAT_BLOCKS, 512) * C + 3 * C) * G


def ba_blocks(nvec):
    return max(1, min(_cdiv(nvec, TD_THREADS * 8), 512))


def ba_workspace_floats(M, C):
    return ba_blocks(M * (C // 8)) * C


# ---- the case tables -------------------------------------------------------------------------------------------------------------------
# S, rps, S_eff, Sq, Q, iters, last: what bn_cut must give (asserted in tests/test_bn_exact_cpu.py); the smallest shapes of each path
BnCase = collections.namedtuple("BnCase", "id Mg C G S rps S_eff Sq Q iters last")
BN_CASES = (
    BnCase("m1", 1, 64, 1, 1, 32, 1, 1, 1, 1, 1),                       # one row; the M = 1 branch of the unbiased variance
    BnCase("m33", 33, 64, 1, 1, 64, 1, 1, 1, 1, 33),                    # the second 32-row slab holds one valid row
    BnCase("m129", 129, 64, 1, 3, 64, 3, 1, 3, 1, 1),
    BnCase("m129g3", 129, 64, 3, 3, 64, 3, 1, 3, 1, 1),                 # groups start inside a split's span in memory
    BnCase("m130", 130, 64, 1, 3, 64, 3, 1, 3, 1, 2),
    BnCase("m130g3", 130, 64, 3, 3, 64, 3, 1, 3, 1, 2),
    BnCase("m2049", 2049, 2048, 1, 16, 160, 13, 1, 13, 2, 129),         # two passes of the row loop, the second with one valid slab
    BnCase("m2050", 2050, 2048, 1, 16, 160, 13, 1, 13, 2, 130),
    BnCase("m1024", 1024, 512, 1, 16, 64, 16, 1, 16, 1, 64),            # either side of bn_stat_splits' wide, short branch
    BnCase("m1026", 1026, 512, 1, 17, 64, 17, 1, 17, 1, 2),
    BnCase("m6145", 6145, 64, 1, 97, 64, 97, 2, 49, 1, 1),              # the smallest shrink; the last shrink block has one row
    BnCase("m6146", 6146, 64, 1, 97, 64, 97, 2, 49, 1, 2),
    BnCase("m32770", 32770, 64, 1, 512, 96, 342, 4, 86, 1, 34),         # the 512 cap; Sq = 4, the last shrink block has two rows
    BnCase("m32770g2", 32770, 64, 2, 512, 96, 342, 4, 86, 1, 34),
    BnCase("m256", 256, 64, 1, 4, 64, 4, 1, 4, 1, 64),                  # a power of two: backward sums that are multiples of Mg
)
BN = {c.id: c for c in BN_CASES}
# td_bn_partial_rows of each case (bn_stat_splits): only m1026 differs from S_eff -- 16 splits of 96 rows, 11 of them used
STAT_ROWS = {c.id: c.S_eff for c in BN_CASES}
STAT_ROWS["m1026"] = 11
GENERAL_IDS = tuple(c.id for c in BN_CASES if c.Mg % 2) + ("m32770",)     # statistics + bounded tiers (and the largest case)
DYADIC_IDS = tuple(c.id for c in BN_CASES if c.Mg % 2 == 0)               # statistics + dyadic tiers
VARIANTS = ((0, False), (1, False), (0, True), (1, True))                 # (relu, residual)

# caller-made partial rows for td_bn_fwd_from_partials / td_bn_bwd_from_partials: (stat_rows, G, Sq, Q, rows of the last shrink block)
# no shrink, the limit, the smallest shrink, Sq = 5 with a full and with a short last block, and 193 rows per shrink block: the
# 12-deep unrolled loop of bn_sum_partials (12 * 16 = 192 rows) runs once and leaves one row to its tail loop
PartCase = collections.namedtuple("PartCase", "R G Sq Q last")
PART_CASES = (PartCase(1, 2, 1, 1, 1), PartCase(96, 2, 1, 96, 1), PartCase(97, 2, 2, 49, 1), PartCase(400, 2, 5, 80, 5),
              PartCase(398, 2, 5, 80, 3), PartCase(18500, 1, 193, 96, 165))
PART_MG, PART_C = 130, 64

# td_bias_act_*: (M, C, blocks of the backward kernel)
BaCase = collections.namedtuple("BaCase", "M C blocks")
BA_CASES = (
    BaCase(1, 8, 1), BaCase(257, 8, 1),
    BaCase(65, 256, 2),                                                   # two blocks, the second with 32 vectors
    BaCase(77, 8, 1), BaCase(77, 16, 1), BaCase(77, 32, 1), BaCase(77, 64, 1), BaCase(77, 128, 1), BaCase(77, 256, 2),
    BaCase(32765, 8, 16), BaCase(32769, 8, 17),                           # the finish kernel's tail loop: one row per slice / two in slice 0
    BaCase(262141, 8, 128), BaCase(262145, 8, 129),                       # its 8-deep loop once in every slice / plus a tail row
    BaCase(131073, 64, 512),                                              # 513 -> 512 blocks: a second grid-stride pass, ragged
)
ACTS = (0, 1, 2)            # none, ELU, leaky ReLU


# ---- float64 replicas of what the kernels compute ---------------------------------------------------------------------------------------

def f32(v):
    """A Python float as the C ABI's `float` parameter holds it."""
    return float(torch.tensor(v, dtype=torch.float32))


def split_sums(v, rps):
    """[G, Mg, C] float64 -> [G, ceil(Mg / rps), C]: column sums over each split's rows."""
    G, Mg, C = v.shape
    return tile_sums(v.reshape(G * Mg, C), G, Mg, rps)


def stats_replica(A, B, count, eps, momentum=None, rm0=None, rv0=None):
    """mean / invstd / running statistics from exact sums A = sum x, B = sum x^2 [G, C] float64 over `count` rows: the operations of
    bn_apply_kernel's prologue and of bn_stats_from_sums_kernel, in double, in their order, each result rounded once to float."""
    assert eps == f32(eps) and (momentum is None or momentum == f32(momentum))
    M = float(count)
    m = A / M
    var = (B / M - m * m).clamp(min=0.0)
    out = types.SimpleNamespace(mean=m.float(), invstd=(1.0 / torch.sqrt(var + eps)).float(), m=m, var=var, rm=None, rv=None)
    if rm0 is not None:
        rm, rv = rm0.double(), rv0.double()
        for grp in range(A.shape[0]):          # one momentum update per group, in order
            unbiased = var[grp] * (M / (M - 1.0)) if M > 1 else var[grp]
            rm = ((1.0 - momentum) * rm + momentum * m[grp]).float().double()
            rv = ((1.0 - momentum) * rv + momentum * unbiased).float().double()
        out.rm, out.rv = rm.float(), rv.float()
    return out


def forward_ref(x, mean, invstd, gamma, beta, res=None, relu=0):
    """y = relu?((x - mean) invstd gamma + beta [+ res]) in float64 from FLOAT mean / invstd [G, C]; x, res [G, Mg, C] float64.
    Returns (y, pre-activation, T) with T the magnitude sum of the forward bound."""
    sc = gamma.double()[None] * invstd.double()
    ms = mean.double() * sc
    pre = x * sc[:, None] + (beta.double()[None] - ms)[:, None]
    T = (x * sc[:, None]).abs() + (ms.abs() + beta.double().abs()[None])[:, None]
    if res is not None:
        pre = pre + res
        T = T + res.abs()
    return (pre.clamp(min=0.0) if relu else pre), pre, T


def backward_ref(gm, x, mean, invstd, gamma, A, B, count):
    """dx = k0 g + k1 x + k2 in float64 (g already masked) from FLOAT mean / invstd and the (global) sums A = sum g,
    B = sum g (x - mean) over `count` rows.  Returns (dx, T) with T the magnitude sum of the backward bound."""
    is_, mu, M = invstd.double(), mean.double(), float(count)
    k0 = gamma.double()[None] * is_
    k1 = -k0 * is_ * (B * is_) / M
    c = k0 * A / M
    dx = k0[:, None] * gm + k1[:, None] * x + (-c - k1 * mu)[:, None]
    T = (k0[:, None] * gm).abs() + (k1[:, None] * x).abs() + ((k1 * mu).abs() + c.abs())[:, None]
    return dx, T


def dgamma_f32(B, invstd):
    """dgamma as the kernels form it: float32 products of the exact B_g and the float invstd_g, added in the order of the groups."""
    t = torch.zeros(B.shape[1])
    for grp in range(B.shape[0]):
        t = t + B[grp].float() * invstd[grp]
    return t


def within_ulps(got, ref, n):
    """got lies within n float32 neighbours of ref, element by element (n = 0: equal)."""
    lo, hi = ref.clone(), ref.clone()
    for _ in range(n):
        lo, hi = torch.nextafter(lo, torch.full_like(lo, -float("inf"))), torch.nextafter(hi, torch.full_like(hi, float("inf")))
    return bool(((got >= lo) & (got <= hi)).all())


def bf16_half_spacing(ref):
    """Half the distance between the bf16 values around each (float64) reference value; 0 at 0."""
    e = torch.frexp(ref)[1]
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 9))


def bound(roundings, T, ref, dtype):
    """The derived bound of the bounded tier for an output stored as `dtype`."""
    b = roundings * U * T
    return b + bf16_half_spacing(ref) if dtype == BF else b


def stored(v, dtype):
    """The float64 reference as an output of `dtype` holds it (one rounding; the tiers that call this have values that survive it)."""
    return bf(v) if dtype == BF else v.float()


def fix_sum(v, cls, target):
    """v [G, R, C] (integers in float64) changed on the LAST rows of the class `cls` (bool [G, R, C]) so that its sum over the class is
    target [G, C]: every row of the class moves by the same q, the last r rows by one more."""
    c = cls.double()
    n = c.sum(1)
    d = target - (v * c).sum(1)
    assert bool(((n > 0) | (d == 0)).all())
    q = torch.floor(d.abs() / n.clamp(min=1.0))
    r = d.abs() - q * n
    from_end = c.flip(1).cumsum(1).flip(1)                 # on a row of the class: its 1-based rank from the end of the class
    out = v + d.sign()[:, None] * (q[:, None] * c + (cls & (from_end <= r[:, None])).double())
    assert torch.equal((out * c).sum(1), target.expand_as(n))
    return out


def _rand_ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def _params(g, C):
    """gamma in {1, 2}, beta a multiple of 0.5, running statistics to start from."""
    return (pick(g, (C,), (1.0, 2.0)), 0.5 * torch.randint(-4, 5, (C,), generator=g).float(),
            torch.randint(-2, 3, (C,), generator=g).float(), pick(g, (C,), (1.0, 0.5, 2.0)))


def _sums(v, w, rps, unit):
    """Exact per-split and per-group sums (sum v, sum v w) with their precondition: [G, S, C, 2], [G, C], [G, C]."""
    check_exact(unit, [v], [v.abs().sum(1)])
    check_exact(unit * unit, [v * w], [(v * w).abs().sum(1)])
    return torch.stack([split_sums(v, rps), split_sums(v * w, rps)], -1), v.sum(1), (v * w).sum(1)


# ---- general integer data: statistics and bounded tiers ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def general_case(cid):
    """Forward operands x (any integers in [-6, 6]) with their exact sums, and backward operands xb (column sums fixed up to an integer
    mean m in {-2 .. 2}), dy, with the float statistics of xb."""
    c = BN[cid]
    g = _gen("bn-general", cid)
    shape = (c.G, c.Mg, c.C)
    gamma, beta, rm0, rv0 = _params(g, c.C)
    x, res, dy = _rand_ints(g, shape, -6, 6), _rand_ints(g, shape, -3, 3), _rand_ints(g, shape, -3, 3)
    m = _rand_ints(g, (c.G, c.C), -2, 2)
    xb = fix_sum(m[:, None] + _rand_ints(g, shape, -3, 3), torch.ones(shape, dtype=torch.bool), m * c.Mg)
    assert float(xb.abs().max()) <= 6 and torch.equal(xb.sum(1) / c.Mg, m)
    out = types.SimpleNamespace(c=c, M=c.G * c.Mg, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, x=x, res=res, dy=dy, xb=xb, m=m)
    for stat in (False, True):            # the cut of td_bn_fwd and the cut of td_bn_fwd_partials
        rps = bn_cut(c.Mg, c.C, stat).rps
        part, A, B = _sums(x, x, rps, 1.0)
        setattr(out, "part_stat" if stat else "part", part)
    out.A, out.B = A, B
    sb = stats_replica(xb.sum(1), (xb * xb).sum(1), c.Mg, EPS)
    assert torch.equal(sb.mean.double(), m)
    out.meanb, out.invstdb = sb.mean, sb.invstd
    return out


def general_forward(cid, relu, with_res, momentum, dtype, count_factor=1):
    """Statistics (exact) and y with its bound for the general data of a case; count_factor 2: two ranks with equal data."""
    d = general_case(cid)
    st = stats_replica(count_factor * d.A, count_factor * d.B, count_factor * d.c.Mg, EPS, momentum, d.rm0, d.rv0)
    y, _, T = forward_ref(d.x, st.mean, st.invstd, d.gamma, d.beta, d.res if with_res else None, relu)
    return st, y, bound(5, T, y, dtype)


def general_backward(cid, relu, with_res, dtype, stat=False, count_factor=1):
    """The backward of the integer-mean data: y_in (the tensor whose sign is the ReLU mask), exact partial rows and sums, dgamma, dbeta,
    dx with its bound, dres."""
    d = general_case(cid)
    c = d.c
    y_in = stored(forward_ref(d.xb, d.meanb, d.invstdb, d.gamma, d.beta, d.res if with_res else None, 1)[0], dtype)
    gm = d.dy * (y_in.double() > 0) if relu else d.dy
    part, A, B = _sums(gm, d.xb - d.m[:, None], bn_cut(c.Mg, c.C, stat).rps, 1.0)
    dx, T = backward_ref(gm, d.xb, d.meanb, d.invstdb, d.gamma, count_factor * A, count_factor * B, count_factor * c.Mg)
    return types.SimpleNamespace(y_in=y_in, gm=gm, part=part, A=A, B=B, dgamma=dgamma_f32(B, d.invstdb), dbeta=A.sum(0).float(),
                                 dx=dx, bound=bound(8, T, dx, dtype))


# ---- dyadic data ----------------------------------------------------------------------------------------------------------------------

def _dyadic(key, Mg, C, G, group_mean=False, multiples=False):
    g = _gen("bn-dyadic", key)
    shape = (G, Mg, C)
    assert Mg % 2 == 0
    gamma, beta, rm0, rv0 = _params(g, C)
    m = _rand_ints(g, (G, 1) if group_mean else (G, C), -2, 2).expand(G, C).contiguous()
    plus = torch.rand(shape, generator=g).argsort(1) < Mg // 2          # m + 1 on exactly half of the rows, in a random order
    sgn = torch.where(plus, 1.0, -1.0).double()
    x = m[:, None] + sgn
    res, dy = _rand_ints(g, shape, -2, 2), _rand_ints(g, shape, -3, 3)
    mean, invstd = m.float(), torch.full((G, C), 0.5)
    out = types.SimpleNamespace(G=G, Mg=Mg, C=C, M=G * Mg, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, x=x, res=res, m=m, mean=mean,
                                invstd=invstd, variants={})
    # sums a multiple of Mg on each sign class (power-of-two Mg): A = (p + n) Mg, B = (p - n) Mg
    p, n = (_rand_ints(g, (G, C), -1, 1) * Mg if multiples else torch.zeros(G, C, dtype=torch.float64) for _ in range(2))
    for relu, with_res in VARIANTS:
        y, pre, _ = forward_ref(x, mean, invstd, gamma, beta, res if with_res else None, relu)
        check_exact(0.5, [y, pre])
        assert torch.equal(bf(y).double(), y)
        if relu:          # the rule of gemm_exact_util._relu_mask: pre-activations that are exactly 0, positive and negative
            assert bool((pre == 0).any()) and bool((pre > 0).any()) and bool((pre < 0).any())
        keep = pre > 0 if relu else torch.ones(shape, dtype=torch.bool)
        gv = dy
        for cls, tgt in ((plus & keep, p), (~plus & keep, n)):
            gv = fix_sum(gv, cls, tgt * (cls.sum(1) >= Mg // 4))         # a class the ReLU leaves few rows of sums to zero
        gm = gv * keep
        SP, SN = (gm * plus).sum(1), (gm * ~plus).sum(1)
        A, B = gm.sum(1), (gm * sgn).sum(1)
        assert torch.equal(A, SP + SN) and torch.equal(B, SP - SN) and float(gv.abs().max()) <= 12
        if not multiples:
            assert not bool(A.any()) and not bool(B.any())
        dx, _ = backward_ref(gm, x, mean, invstd, gamma, A, B, Mg)
        check_exact(0.125, [dx])
        assert float(dx.abs().max()) < 16 and torch.equal(bf(dx).double(), dx)
        if not multiples:
            assert torch.equal(dx, gm * (gamma.double() * 0.5))
        out.variants[(relu, with_res)] = types.SimpleNamespace(y=y, dy=gv, gm=gm, A=A, B=B, dx=dx, dgamma=dgamma_f32(B, invstd),
                                                               dbeta=A.sum(0).float())
    return out


@functools.lru_cache(maxsize=2)
def dyadic_case(cid):
    c = BN[cid]
    d = _dyadic(cid, c.Mg, c.C, c.G, multiples=(cid == "m256"))
    d.c = c
    for stat in (False, True):
        part, A, B = _sums(d.x, d.x, bn_cut(c.Mg, c.C, stat).rps, 1.0)
        setattr(d, "part_stat" if stat else "part", part)
    d.A, d.B = A, B
    assert torch.equal(A / c.Mg, d.m) and torch.equal(B / c.Mg - d.m * d.m, torch.ones_like(A))
    return d


def dyadic_stats(d, momentum, count_factor=1):
    st = stats_replica(count_factor * d.A, count_factor * d.B, count_factor * d.Mg, EPS_DYADIC, momentum, d.rm0, d.rv0)
    assert torch.equal(st.mean, d.mean) and torch.equal(st.invstd, d.invstd)
    return st


def backward_partials(d, v, stat=False):
    """Exact per-split rows (sum g, sum g (x - m)) of a dyadic case's variant."""
    return _sums(v.gm, d.x - d.m[:, None], bn_cut(d.Mg, d.C, stat).rps, 1.0)[0]


@functools.lru_cache(maxsize=None)
def partials_case(i):
    """Dyadic data whose statistics reach the kernels as caller-made partial rows (fabricate_partials: one target per group, so the mean
    is the group's): forward rows that sum to (m Mg, (m^2 + 1) Mg), backward rows that sum to zero."""
    pc = PART_CASES[i]
    d = _dyadic(("partials", i), PART_MG, PART_C, pc.G, group_mean=True)
    g = _gen("bn-partials", i)
    mg = d.m[:, 0]
    d.pc = pc
    d.part_fwd = fabricate_partials(g, pc.G, pc.R, PART_C, mg * PART_MG, (mg * mg + 1) * PART_MG)
    d.part_bwd = fabricate_partials(g, pc.G, pc.R, PART_C, torch.zeros(pc.G), torch.zeros(pc.G))
    d.A, d.B = d.x.sum(1), (d.x * d.x).sum(1)
    assert torch.equal(d.part_fwd.double().sum(1)[..., 0], d.A) and torch.equal(d.part_fwd.double().sum(1)[..., 1], d.B)
    return d


# ---- bias + activation ------------------------------------------------------------------------------------------------------------------

def leaky_f32(v):
    """v > 0 ? v : 0.01f * v with the float32 product, as float64."""
    return torch.where(v > 0, v, (LEAKY * v.float()).double())


@functools.lru_cache(maxsize=4)
def ba_case(M, C, act, masked_grads=False):
    """Operands and references of td_bias_act_fwd / td_bias_act_bwd.  Forward (act none, leaky): integers y + bias.  Backward: the
    result `a` is an INPUT, so it is fabricated -- ELU: positive integers and negatives in {-0.5, -0.75}, so gy = g (a + 1) is a
    multiple of 0.25; leaky: the forward's own result, and where a <= 0 the gradient is 0 (masked_grads: any integer; then dbias is
    not an exact sum)."""
    g = _gen("bias-act", M, C, act, masked_grads)
    y, bias, up = _rand_ints(g, (M, C), -3, 3), _rand_ints(g, (C,), -2, 2), _rand_ints(g, (M, C), -3, 3)
    z = y + bias
    out = types.SimpleNamespace(M=M, C=C, act=act, y=y, bias=bias, fwd=None)
    if act == 0:
        out.fwd, a, gy = z, None, up
    elif act == 1:
        a = torch.where(torch.rand(M, C, generator=g) < 0.5, _rand_ints(g, (M, C), 1, 3), pick(g, (M, C), (-0.5, -0.75)).double())
        gy = torch.where(a > 0, up, up * (a + 1.0))
    else:
        out.fwd = a = leaky_f32(z)
        if not masked_grads:
            up = up * (a > 0)
        gy = leaky_f32_grad(up, a)
    out.a, out.up, out.gy = a, up, gy
    out.exact = not masked_grads
    if out.exact:
        check_exact(0.25, [gy], [gy.abs().sum(0)])
    out.dbias, out.abs_sum = gy.sum(0), float(gy.abs().sum(0).max())
    return out


def leaky_f32_grad(up, a):
    return torch.where(a > 0, up, (LEAKY * up.float()).double())
