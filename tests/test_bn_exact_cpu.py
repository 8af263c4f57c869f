"""The cases of tests/test_hip_bn_exact.py without a GPU: every case of the tables in tests/bn_exact_util.py reaches the path it is named
for (by the replicas of the host-side cut functions, which are also held against the library's own td_bn_partial_rows,
td_bn_workspace_floats and td_bias_act_workspace_floats: host functions, they load on a CPU-only machine), every builder's exactness
preconditions hold (the builders assert them on the reference alone), the dyadic and zero-sum constructions produce what they claim,
and the float64 replicas ARE the operation: they agree with float64 autograd of F.batch_norm -> add -> relu, F.elu and F.leaky_relu
to float64 round-off (1e-12 of the largest magnitude)."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_exact_util as E

RTOL = 1e-12


def _lib():
    import tripled_amd  # noqa: F401
    from tripled_amd import native
    return native.load()


def _close(got, ref, what):
    assert float((got - ref).abs().max()) <= RTOL * max(1.0, float(ref.abs().max())), what


# ---- the paths -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", E.BN_CASES, ids=[c.id for c in E.BN_CASES])
def test_batchnorm_cases_reach_their_paths(c):
    lib = _lib()
    cut = E.bn_cut(c.Mg, c.C)
    assert (cut.S, cut.rps, cut.S_eff, cut.Sq, cut.Q, cut.iters, cut.last) == c[4:]
    assert (c.Sq > 1) == (c.S_eff > E.BN_PRO_MAX_S) and c.Q <= E.BN_PRO_MAX_S and 0 < c.last <= c.rps
    M = c.Mg * c.G
    assert lib.td_bn_workspace_floats(M, c.G, c.C) == E.bn_workspace_floats(M, c.G, c.C) >= 2 * c.S_eff * c.C * c.G
    assert lib.td_bn_partial_rows(M, c.G, c.C) == E.bn_cut(c.Mg, c.C, stat=True).S_eff == E.STAT_ROWS[c.id]


def test_batchnorm_table_covers_what_it_claims():
    B = E.BN
    assert B["m1"].Mg == 1 and B["m33"].rps == 64 and B["m33"].last - 32 == 1                 # one valid row in the second slab
    for a, b in (("m129", "m130"), ("m129g3", "m130g3")):
        assert (B[a].S_eff, B[a].last, B[b].last) == (3, 1, 2)
    assert B["m129g3"].G == 3 and B["m129g3"].Mg % B["m129g3"].rps != 0                       # groups start inside a split's span
    for cid in ("m2049", "m2050"):      # 16 splits of 160 rows: two passes, the prefetch fires, the second pass holds one slab
        c = B[cid]
        assert (c.C, c.S, c.rps, c.iters) == (2048, 16, 160, 2) and c.rps - E.BN_RY * E.BN_UNROLL == E.BN_RY
    # either side of the wide, short branch of bn_stat_splits: 16 splits as they are; 17 -> 16 splits of 96 rows (11 used)
    assert (B["m1024"].S, E.bn_stat_splits(1024, 512), E.STAT_ROWS["m1024"]) == (16, 16, 16)
    assert (B["m1026"].S, E.bn_stat_splits(1026, 512), E.bn_cut(1026, 512, True).rps, E.STAT_ROWS["m1026"]) == (17, 16, 96, 11)
    assert E.STAT_ROWS["m1026"] != B["m1026"].S_eff
    for cid, last in (("m6145", 1), ("m6146", 2)):
        c = B[cid]
        assert (c.S_eff, c.Sq, c.Q, c.last) == (97, 2, 49, last) and c.S_eff - (c.Q - 1) * c.Sq == 1      # last shrink block: one row
    c = B["m32770"]
    assert (c.S, c.rps, c.S_eff, c.Sq, c.Q) == (512, 96, 342, 4, 86) and c.Sq < E.BN_FIN_PARTS            # bn_sum_partials: tail loop only
    assert 36 * 32770 < 2 ** 24 and B["m32770g2"].G == 2
    assert B["m256"].Mg & (B["m256"].Mg - 1) == 0
    assert set(E.GENERAL_IDS) | set(E.DYADIC_IDS) == set(B) and all(B[i].Mg % 2 for i in E.GENERAL_IDS if i != "m32770")
    assert max(c.Mg * c.G * c.C for c in E.BN_CASES) == 2050 * 2048                                        # the largest tensor: 8 MB bf16


@pytest.mark.parametrize("pc", E.PART_CASES, ids=[str(pc.R) for pc in E.PART_CASES])
def test_partial_row_cases_reach_their_shrinks(pc):
    assert E.bn_shrink(pc.R) == (pc.Sq, pc.Q) and pc.R - (pc.Q - 1) * pc.Sq == pc.last
    assert pc.Q <= E.BN_PRO_MAX_S
    if pc.R == 18500:       # 12 loads in flight in each of the 16 slices, then a tail row in slice 0; the short last block: tail loop only
        assert pc.Sq == 12 * E.BN_FIN_PARTS + 1 and pc.last <= 11 * E.BN_FIN_PARTS
    assert {p.R for p in E.PART_CASES} >= {1, 96, 97, 400} and any(p.Sq == 5 and p.last < p.Sq for p in E.PART_CASES)


@pytest.mark.parametrize("c", E.BA_CASES, ids=["%dx%d" % c[:2] for c in E.BA_CASES])
def test_bias_act_cases_reach_their_blocks(c):
    nvec = c.M * (c.C // 8)
    assert E.ba_blocks(nvec) == c.blocks
    assert _lib().td_bias_act_workspace_floats(c.M, c.C) == E.ba_workspace_floats(c.M, c.C) == c.blocks * c.C


def test_bias_act_table_covers_what_it_claims():
    cases = {(c.M, c.C): c for c in E.BA_CASES}
    assert {(1, 8), (257, 8), (65, 256), (131073, 64)} <= set(cases)
    assert 65 * 32 - 2048 == 32                                               # the second block holds 32 vectors
    assert {c.C for c in E.BA_CASES if c.M == 77} == {8, 16, 32, 64, 128, 256}
    assert {c.blocks for c in E.BA_CASES} >= {16, 17, 128, 129, 512}
    nvec = 131073 * 8
    assert -(-nvec // 2048) == 513 and nvec % (512 * 256) == 8                # capped; the last grid-stride pass holds 8 vectors
    assert all(c.M % 2 for c in E.BA_CASES)


# ---- preconditions and constructions -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", E.GENERAL_IDS)
def test_general_cases_are_exact(cid):
    """Builds the case (the builder asserts that every sum is an fp32 value in any order) and each backward variant."""
    d = E.general_case(cid)
    c = d.c
    assert d.part.shape == (c.G, c.S_eff, c.C, 2) and d.part_stat.shape[1] == E.STAT_ROWS[cid]
    assert torch.equal(d.part.sum(1), torch.stack([d.A, d.B], -1)) and float(d.B.max()) < 2 ** 24
    assert float(d.x.abs().max()) <= 6 and float(d.xb.abs().max()) <= 6
    assert torch.equal(d.meanb.double() * c.Mg, d.xb.sum(1))                   # an integer mean: g (x - mean) stays an integer
    assert bool(((d.m == 0) | (d.m.abs() == 1) | (d.m.abs() == 2)).all())     # 0 or a power of two: k1 * mean is exact
    for relu, with_res in E.VARIANTS:
        b = E.general_backward(cid, relu, with_res, E.BF)
        assert torch.equal(b.part.sum(1), torch.stack([b.A, b.B], -1)) and bool((b.bound < 2.0 ** -5).all())
        if relu and c.Mg > 1:
            assert bool((b.gm != d.dy).any())


@pytest.mark.parametrize("cid", E.DYADIC_IDS)
def test_dyadic_cases_produce_what_they_claim(cid):
    d = E.dyadic_case(cid)
    c = d.c
    assert torch.equal(d.x.sum(1) / c.Mg, d.m) and torch.equal(((d.x - d.m[:, None]) ** 2).sum(1) / c.Mg, torch.ones(c.G, c.C, dtype=torch.float64))
    for momentum in (0.25, E.MOMENTUM_TENTH):
        st = E.dyadic_stats(d, momentum)                                      # asserts mean == m and invstd == 0.5 through the replica
        assert st.rm.dtype == torch.float32
    for (relu, with_res), v in d.variants.items():
        assert torch.equal(v.gm.sum(1), v.A) and torch.equal((v.gm * (d.x - d.m[:, None])).sum(1), v.B)
        if cid == "m256":
            assert bool(v.A.any()) and bool(v.B.any()) and not bool((v.A % c.Mg).any()) and not bool((v.B % c.Mg).any())
            assert bool((v.dx % 0.5 != 0).any())                              # the eighths are really used
        else:
            assert not bool(v.A.any()) and not bool(v.B.any())
            assert torch.equal(v.dx, v.gm * (d.gamma.double() * 0.5))
        assert bool((v.y % 1 == 0.5).any())


@pytest.mark.parametrize("i", range(len(E.PART_CASES)))
def test_fabricated_partial_rows_sum_to_the_statistics(i):
    d = E.partials_case(i)
    pc = d.pc
    assert d.part_fwd.shape == d.part_bwd.shape == (pc.G, pc.R, E.PART_C, 2)
    s = d.part_fwd.double().sum(1)
    st = E.stats_replica(s[..., 0], s[..., 1], E.PART_MG, E.EPS_DYADIC)
    assert torch.equal(st.mean, d.mean) and torch.equal(st.invstd, d.invstd)
    assert not bool(d.part_bwd.double().sum(1).any()) and (pc.R == 1 or bool(d.part_bwd.any()))


def test_helpers_refuse_what_is_wrong():
    one = torch.tensor([1.0])
    assert E.within_ulps(one + 2.0 ** -22, one, 2) and not E.within_ulps(one + 2.0 ** -22, one, 1) and E.within_ulps(one, one, 0)
    assert float(E.bf16_half_spacing(torch.tensor([1.5], dtype=torch.float64))) == 2.0 ** -8
    assert float(E.bf16_half_spacing(torch.tensor([0.0], dtype=torch.float64))) == 0.0
    v = torch.zeros(1, 5, 1, dtype=torch.float64)
    out = E.fix_sum(v, torch.tensor([1, 0, 1, 1, 0], dtype=torch.bool).reshape(1, 5, 1), torch.tensor([[-5.0]]))
    assert out.flatten().tolist() == [-1, 0, -2, -2, 0]
    with pytest.raises(AssertionError):
        E.fix_sum(v, torch.zeros(1, 5, 1, dtype=torch.bool), torch.tensor([[1.0]]))


# ---- the replicas against the operation itself --------------------------------------------------------------------------------------------

def _autograd(x, res, dy, gamma, beta, eps, relu):
    """float64 autograd of F.batch_norm -> add -> relu, group by group; the running statistics with momentum 1: the batch's own."""
    G, Mg, C = x.shape
    w, b = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ys, dxs, drs, means, unbiased = [], [], [], [], []
    for grp in range(G):
        xg = x[grp].clone().requires_grad_(True)
        rg = res[grp].clone().requires_grad_(True) if res is not None else None
        rm, rv = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
        y = F.batch_norm(xg, rm, rv, w, b, True, 1.0, eps)
        y = y + rg if rg is not None else y
        y = F.relu(y) if relu else y
        y.backward(dy[grp])
        ys.append(y.detach()), dxs.append(xg.grad), drs.append(rg.grad if rg is not None else None), means.append(rm), unbiased.append(rv)
    return torch.stack(ys), torch.stack(dxs), (torch.stack(drs) if res is not None else None), w.grad, b.grad, torch.stack(means), torch.stack(unbiased)


@pytest.mark.parametrize("relu,with_res", E.VARIANTS)
@pytest.mark.parametrize("cid", ("m33", "m129g3", "m6145", "m130g3", "m256"))
def test_replicas_agree_with_float64_autograd(cid, relu, with_res):
    c = E.BN[cid]
    if cid in E.GENERAL_IDS:
        d = E.general_case(cid)
        x, dy, eps = d.x, d.dy, E.EPS
    else:
        d = E.dyadic_case(cid)
        x, dy, eps = d.x, d.variants[(relu, with_res)].dy, E.EPS_DYADIC
    res = d.res if with_res else None
    st = E.stats_replica(x.sum(1), (x * x).sum(1), c.Mg, eps)
    mean, invstd = st.m, 1.0 / torch.sqrt(st.var + eps)                      # the replica's statistics before their rounding to float
    y, pre, _ = E.forward_ref(x, mean, invstd, d.gamma, d.beta, res, relu)
    gm = dy * (pre > 0) if relu else dy
    A, B = gm.sum(1), (gm * (x - mean[:, None])).sum(1)
    dx, _ = E.backward_ref(gm, x, mean, invstd, d.gamma, A, B, c.Mg)
    ry, rdx, rdres, rdw, rdb, rmean, runb = _autograd(x, res, dy, d.gamma, d.beta, eps, relu)
    _close(y, ry, "y")
    _close(dx, rdx, "dx")
    if with_res:
        _close(gm, rdres, "dres")
    _close((B * invstd).sum(0), rdw, "dgamma")
    _close(A.sum(0), rdb, "dbeta")
    _close(mean, rmean, "batch mean")
    _close(st.var * (c.Mg / (c.Mg - 1.0)), runb, "unbiased variance")
    # the float results are those values rounded once
    assert torch.equal(st.mean, mean.float()) and torch.equal(st.invstd, invstd.float())
    dg32 = E.dgamma_f32(B.float().double(), invstd.float())
    # G float32 products of a rounded B and a rounded invstd, G float32 additions
    assert float((dg32.double() - rdw).abs().max()) <= (4 * c.G) * E.U * float((B * invstd).abs().sum(0).max()) + 1e-30


def test_running_statistics_replica_is_the_momentum_update():
    d = E.general_case("m129g3")
    for momentum in (0.25, E.MOMENTUM_TENTH):
        st = E.stats_replica(d.A, d.B, d.c.Mg, E.EPS, momentum, d.rm0, d.rv0)
        rm, rv = d.rm0.double(), d.rv0.double()
        for grp in range(d.c.G):
            xg = d.x[grp]
            F.batch_norm(xg, rm, rv, None, None, True, momentum, E.EPS)         # updates rm, rv in place, in float64
        # three updates, each rounded to float by the replica: 3 float roundings away from the unrounded float64 recursion
        assert float((st.rm.double() - rm).abs().max()) <= 3 * 2.0 ** -24 * float(rm.abs().max() + 1)
        assert float((st.rv.double() - rv).abs().max()) <= 3 * 2.0 ** -24 * float(rv.abs().max() + 1)
    one = E.stats_replica(d.A[:1] * 0 + 3.0, d.B[:1] * 0 + 9.0, 1, E.EPS, 0.25, d.rm0, d.rv0)          # M = 1: var 0, not unbiased
    assert torch.equal(one.rv, (0.75 * d.rv0.double()).float()) and torch.equal(one.mean, torch.full_like(one.mean, 3.0))


@pytest.mark.parametrize("act", E.ACTS)
def test_bias_act_replicas_agree_with_float64_autograd(act):
    """Leaky ReLU: the reference holds the FLOAT32 product 0.01f * v, one float32 rounding (2^-24 relative) away from float64's."""
    M, C = 257, 8
    slope = float(E.LEAKY)
    fn = {0: lambda z: z, 1: F.elu, 2: lambda z: F.leaky_relu(z, slope)}[act]

    def close(got, ref, what):
        if act == 2:
            assert bool(((got - ref).abs() <= E.U * ref.abs()).all()), what
        else:
            _close(got, ref, what)
    for masked in ((False, True) if act == 2 else (False,)):
        r = E.ba_case(M, C, act, masked)
        if act != 1:
            close(r.fwd, fn(r.y + r.bias), "forward")
            z = (r.y + r.bias).requires_grad_(True)
        else:       # the fabricated result a = elu(z) for z = a (a > 0), log1p(a) (a < 0)
            z = torch.where(r.a > 0, r.a, torch.log1p(r.a.clamp(max=0.0))).requires_grad_(True)
            _close(fn(z).detach(), r.a, "fabricated ELU result")
        fn(z).backward(r.up)
        close(r.gy, z.grad, "gy")
        if r.exact:
            _close(r.dbias, z.grad.sum(0), "dbias")
            assert act != 2 or bool((r.up[r.a <= 0] == 0).all())
        else:
            assert bool((r.up[r.a <= 0] != 0).any())
