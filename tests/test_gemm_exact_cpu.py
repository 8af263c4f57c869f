"""The cases of tests/test_hip_gemm_exact.py without a GPU: every case of the tables in tests/gemm_exact_util.py is built (operands and
float64 reference; the builders assert the exactness preconditions on the reference alone -- all values multiples of one power of
two u, every sum the kernels form with sum |terms| < 2^24 u), and the tile height, split count and stage counts each case is meant
to reach are pinned through the library's host functions (td_conv1x1_stat_rows, td_conv1x1_wgrad_workspace_floats,
td_conv3x3_wgrad_workspace_floats), which load on a CPU-only host.  The tile WIDTH (64 or 128 columns) is not observable from
outside: it is pinned against gemm_exact_util.pick_tile, the three-line replica of cv_pick_tile (csrc/td_conv_tile.h)."""
import pytest
import torch

from tests import gemm_exact_util as E


def _lib():
    import tripled_amd  # noqa: F401
    from tripled_amd import native
    return native.load()


@pytest.mark.parametrize("rc", E.ROW_CASES, ids=[rc.id for rc in E.ROW_CASES])
def test_row_cases_reach_their_tiles(rc):
    lib = _lib()
    assert E.pick_tile(rc.Mg, rc.G, rc.width) == (rc.bm, rc.bn)
    S = -(-rc.Mg // rc.bm)
    assert lib.td_conv1x1_stat_rows(rc.Mg * rc.G, rc.G, rc.width) == S
    assert rc.Mg - (S - 1) * rc.bm == rc.last and rc.last < rc.bm             # ragged
    # the fused data gradient demotes 128 x 128 by design; deep pipelines: 64 x 64 always, 128 x 64 without a prologue
    assert E.dispatched(rc, 192, prologue=2)[:2] == (rc.bm, 64 if rc.bm == 128 else rc.bn)
    assert [E.dispatched(rc, k)[2] for k in (64, 128, 192, 320)] == [False, False, rc.bn == 64, rc.bn == 64]
    assert E.dispatched(rc, 320, prologue=1)[2] == (rc.bm == 64)
    assert all(k % 64 == 0 and k <= 512 for k in E.REDUCTIONS[rc.id])        # the fused prologues' limit
    assert E.dispatched(rc, 192)[2] or set(E.REDUCTIONS[rc.id]) == {64, 192}


def test_tables_cover_what_they_claim():
    tiles = {(rc.bm, rc.bn) for rc in E.ROW_CASES}
    assert tiles == {(64, 64), (128, 64), (128, 128)}
    assert {rc.last for rc in E.ROW_CASES if rc.bm == 128} >= {1, 33, 65}     # either side of the lr + 32 and lr + 64 stores
    assert max(rc.G for rc in E.ROW_CASES) == 64 and any(rc.G > 1 and rc.Mg % rc.bm for rc in E.ROW_CASES)
    assert len(E.GEMM_COMBOS) == 24
    used = {E.in_rows_for(*c) for c in E.GEMM_COMBOS}, {E.in_rows_for(*c, shift=2) for c in E.GEMM_COMBOS}
    assert used == (set(E.IN_ROWS), set(E.IN_ROWS))
    assert max(rc.Mg * rc.G * max(E.REDUCTIONS[rc.id]) for rc in E.ROW_CASES) == 57408 * 320       # the largest operand: 37 MB


@pytest.mark.parametrize("rid,red", E.GEMM_COMBOS, ids=["%s-k%d" % c for c in E.GEMM_COMBOS])
def test_gemm_cases_are_exact(rid, red):
    """Builds the four references of the shape (each builder asserts its preconditions) and checks what the GPU test relies on."""
    rc = E.ROWS[rid]
    f = E.forward_case(rid, red)
    assert f.y.shape == (f.M, rc.width) and f.stats.shape == (rc.G, -(-rc.Mg // rc.bm), rc.width, 2)
    rows = f.y.double().reshape(rc.G, rc.Mg, -1)
    assert torch.equal(f.stats.sum(1), torch.stack([rows.sum(1), (rows * rows).sum(1)], -1))
    assert float(f.y.double().abs().max()) <= 3 * red and float(f.stats[..., 1].max()) < E.LIMIT
    assert not torch.equal(f.run_out, f.y)
    d = E.dgrad_case(rid, red)
    assert d.dx.shape == (d.M, rc.width) and d.sums.shape == f.stats.shape and not torch.equal(d.dx_res, d.dx)
    a = E.bnrelu_case(rid, red, E.in_rows_for(rid, red))
    assert a.part.shape == (rc.G, a.in_rows, red, 2) and a.a.shape == (a.M, red) and float(a.a.min()) == 0
    # the fabricated partial rows give mean m_g = 2 + g and variance 0.5 in double, exactly
    A, B = a.part.double().sum(1)[..., 0], a.part.double().sum(1)[..., 1]
    assert torch.equal(A / rc.Mg, a.mean.double()) and torch.equal(B / rc.Mg - (A / rc.Mg) ** 2, torch.full_like(A, 0.5))
    b = E.bnbwd_case(rid, red, E.in_rows_for(rid, red, shift=2))
    assert b.dz.shape == (b.M, red) and b.dx.shape == (b.M, rc.width) and not bool(b.part.any())
    assert bool((b.dz.double() % 1 == 0.5).any())                              # the half-integer unit is really used


@pytest.mark.parametrize("case", [c + (N,) for c in E.STRIDE2_CASES for N in (64, 128)])
def test_stride2_cases_are_exact(case):
    s = E.stride2_case(*case)
    B, Hi, Wi, groups, N = case
    assert s.x.shape == (B * Hi * Wi, 64) and s.y.shape == (s.M, N) and s.M % groups == 0
    assert _lib().td_conv1x1_stat_rows(s.M, groups, N) == 1 == s.stats.shape[1]


@pytest.mark.parametrize("i", range(len(E.WGRAD_CASES)))
def test_weight_gradient_cases_reach_their_splits(i):
    c = E.WGRAD_CASES[i]
    assert _lib().td_conv1x1_wgrad_workspace_floats(c.M, c.K, c.N) == c.P * c.N * c.K
    assert E.split_ranges(c.M, (c.N // 64) * (c.K // 64), 768) == (c.P, c.stages)
    w = E.wgrad_case(i)
    assert w.dw.shape == (c.N, c.K) and w.x.shape == (c.B * c.Hi * c.Wi, c.K)
    assert float(w.dw.abs().max()) < E.LIMIT


def test_weight_gradient_table_covers_the_prefetch_special_cases():
    stages = {s for c in E.WGRAD_CASES for s in c.stages}
    assert stages >= {1, 2, 3} and any(len(c.stages) < c.P for c in E.WGRAD_CASES)    # P_eff < P
    assert {s for c in E.W3_CASES for s in c.stages} >= {2, 3}


@pytest.mark.parametrize("i", range(len(E.CONV3_CASES)))
def test_conv3x3_cases_are_exact(i):
    c = E.CONV3_CASES[i]
    r = E.conv3_case(i)
    assert E.pick_tile(r.rc.Mg, c.groups, c.N) == (c.bm, c.bn)
    assert _lib().td_conv1x1_stat_rows(r.M, c.groups, c.N) == -(-r.rc.Mg // c.bm) == r.stats.shape[1]
    assert r.rc.Mg % c.bm != 0 and r.y.shape == (r.M, c.N)


@pytest.mark.parametrize("pad", (0, 1))
@pytest.mark.parametrize("i", range(len(E.W3_CASES)))
def test_conv3x3_weight_gradient_cases_reach_their_splits(i, pad):
    c = E.W3_CASES[i]
    assert _lib().td_conv3x3_wgrad_workspace_floats(c.B, c.Ho, c.Wo, c.C, c.N) == c.P * c.N * 9 * c.C
    assert E.split_ranges(c.B * c.Ho * c.Wo, (c.N // 64) * (c.C // 64), 256) == (c.P, c.stages)
    r = E.w3_case(i, pad)
    assert r.dw.shape == (c.N, 3, 3, c.C) and float(r.dw.abs().max()) < E.LIMIT


def test_check_exact_refuses_what_is_not_exact():
    E.check_exact(0.5, [torch.tensor([1.5, -2.0])], [torch.tensor([2.0 ** 23 - 1])])
    with pytest.raises(AssertionError):
        E.check_exact(1.0, [torch.tensor([1.5])])
    with pytest.raises(AssertionError):
        E.check_exact(0.5, [], [torch.tensor([2.0 ** 23])])
    with pytest.raises(AssertionError):
        E.check_exact(1.0, [torch.tensor([float("nan")])])
    assert E.one_ulp(torch.tensor([1.0, 1.0 + 2.0 ** -23]), torch.tensor([1.0, 1.0]))
    assert not E.one_ulp(torch.tensor([1.0 + 2.0 ** -22]), torch.tensor([1.0]))
