"""The MFMA GEMM kernel family (csrc/td_conv1x1.hip, td_conv3x3.hip, td_conv3x3_wgrad.hip, td_conv_tile.h) on small integer operands,
where fp32 accumulation is exact in any order: every output equals the float64 reference, rounded to bf16 where the kernel rounds,
BIT FOR BIT (torch.equal; -0 equals +0), and so do the epilogue statistics, tile by tile.  The cases (tests/gemm_exact_util.py; their
preconditions and the tiles they reach are proven in tests/test_gemm_exact_cpu.py) are the edges the workload's own shapes never run:
ragged 128-row tiles (1, 33 and 65 valid rows), groups that start inside a tile's span, 64 groups, an odd number of K stages in the
deep pipeline (192, 320), two stages on few rows, weight gradients of one, two and three stages and with trailing row ranges that
are not launched, 3x3 convolutions of one output pixel, of stride 2 without padding and of 8 channels on 128-row tiles.

Every operand lies between NaN guard rows (a read past the end that reaches the arithmetic poisons the result), every output is
pre-filled with NaN between guard rows of a marker: afterwards no NaN is left and the guards are untouched.  The only comparison
that is not exact is the running statistics of td_conv1x1_fwd_bnrelu (one float32 ulp: the compiler may fuse the double
multiply-add)."""
import ctypes

import pytest
import torch

from tests import gemm_exact_util as E

pytestmark = pytest.mark.gpu

_IDS = ["%s-k%d" % c for c in E.GEMM_COMBOS]


@pytest.fixture(scope="module", params=E.GEMM_COMBOS, ids=_IDS)
def combo(request):
    """Module scope: pytest runs all tests of one (row case, reduction width) together, so the cached references are built once."""
    return request.param


def _lib():
    import tripled_amd  # noqa: F401
    from tripled_amd import native
    return native.load(), native


def _stat_buffer(lib, M, G, N, bm):
    S = lib.td_conv1x1_stat_rows(M, G, N)
    assert S == -(-(M // G) // bm)
    return E.fenced(G * S, N * 2, torch.float32, E.MARKER), S


def _assert_stats(f, ref, what):
    """Partial rows: all finite, each equal to the sums over the rows of its own tile, and (hence) their float64 totals to the group's."""
    E.assert_fence(f, what)
    got = f.view.double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got.sum(1), ref.sum(1)), what + ": totals"
    assert torch.equal(got, ref), what + ": per tile"


def _assert_rows(f, ref, what):
    E.assert_fence(f, what)
    assert torch.equal(f.view.cpu(), ref), what


# ---- td_conv1x1_fwd, td_conv1x1_fwd_sum -----------------------------------------------------------------------------------------------

def _run_fwd(c, stride=1, Hi=0, Wi=0, stats=True):
    lib, native = _lib()
    rc, K = c.rc, c.x.shape[1]
    x, w = E.fenced_input(c.x), E.fenced_input(c.w)
    y = E.fenced_output(c.M, rc.width)
    st, _ = _stat_buffer(lib, c.M, rc.G, rc.width, rc.bm) if stats else (None, 0)
    native.check(lib.td_conv1x1_fwd(native.ptr(x), native.ptr(w), c.M, rc.G, K, rc.width, Hi, Wi, stride, native.ptr(y.view),
                                    native.ptr(st.view) if stats else None, native.stream()), "td_conv1x1_fwd")
    torch.cuda.synchronize()
    _assert_rows(y, c.y, "y")
    if stats:
        _assert_stats(st, c.stats, "stat_partials")


def test_forward_and_epilogue_statistics(combo):
    _run_fwd(E.forward_case(*combo))


def test_forward_without_statistics():
    _run_fwd(E.forward_case("r4", 192), stats=False)          # 128 x 64, deep, 33 valid rows in the last tile


@pytest.mark.parametrize("case", [c + (N,) for c in E.STRIDE2_CASES for N in (64, 128)])
def test_forward_stride2(case):
    _run_fwd(E.stride2_case(*case), stride=2, Hi=case[1], Wi=case[2])


def test_forward_with_running_sum(combo):
    """td_conv1x1_fwd_sum takes no groups: the rows of all groups as one (its own tile choice; the reference does not depend on it)."""
    lib, native = _lib()
    c = E.forward_case(*combo)
    rc, K = c.rc, combo[1]
    x, w, run_in = E.fenced_input(c.x), E.fenced_input(c.w), E.fenced_input(c.run_in)
    y, run_out = E.fenced_output(c.M, rc.width), E.fenced_output(c.M, rc.width)
    native.check(lib.td_conv1x1_fwd_sum(native.ptr(x), native.ptr(w), c.M, K, rc.width, native.ptr(run_in), native.ptr(y.view),
                                        native.ptr(run_out.view), native.stream()), "td_conv1x1_fwd_sum")
    torch.cuda.synchronize()
    _assert_rows(y, c.y, "y")
    _assert_rows(run_out, c.run_out, "run_out")


# ---- td_conv1x1_dgrad, td_conv1x1_dgrad_bnsums ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_res", (False, True))
def test_data_gradient(combo, with_res):
    lib, native = _lib()
    c = E.dgrad_case(*combo)
    rc, Cout = c.rc, combo[1]
    dy, w = E.fenced_input(c.dy), E.fenced_input(c.w)
    res = E.fenced_input(c.res) if with_res else None
    dx = E.fenced_output(c.M, rc.width)
    native.check(lib.td_conv1x1_dgrad(native.ptr(dy), native.ptr(w), c.M, rc.G, Cout, rc.width, native.ptr(res), native.ptr(dx.view),
                                      native.stream()), "td_conv1x1_dgrad")
    torch.cuda.synchronize()
    _assert_rows(dx, c.dx_res if with_res else c.dx, "dx")


def test_data_gradient_with_backward_sums(combo):
    lib, native = _lib()
    c = E.dgrad_case(*combo)
    rc, Cout = c.rc, combo[1]
    dy, w, z = E.fenced_input(c.dy), E.fenced_input(c.w), E.fenced_input(c.z)
    dx = E.fenced_output(c.M, rc.width)
    out, _ = _stat_buffer(lib, c.M, rc.G, rc.width, rc.bm)
    gamma, beta, mean, invstd = c.gamma.cuda(), c.beta.cuda(), c.mean.cuda(), c.invstd.cuda()
    native.check(lib.td_conv1x1_dgrad_bnsums(native.ptr(dy), native.ptr(w), c.M, rc.G, Cout, rc.width, native.ptr(z), native.ptr(gamma),
                                             native.ptr(beta), native.ptr(mean), native.ptr(invstd), native.ptr(dx.view),
                                             native.ptr(out.view), native.stream()), "td_conv1x1_dgrad_bnsums")
    torch.cuda.synchronize()
    _assert_rows(dx, c.dx, "dx")
    _assert_stats(out, c.sums, "out_partials")


# ---- td_conv1x1_fwd_bnrelu ------------------------------------------------------------------------------------------------------------

def _run_bnrelu(c):
    lib, native = _lib()
    rc, K = c.rc, c.z.shape[1]
    z, w = E.fenced_input(c.z), E.fenced_input(c.w)
    part = E.fenced_input(c.part.reshape(rc.G * c.in_rows, K * 2))          # reduced in place by the call
    gamma, beta, rm, rv = c.gamma.cuda(), c.beta.cuda(), c.rm0.cuda(), c.rv0.cuda()
    mean, invstd = (torch.full((rc.G, K), E.NAN, device="cuda") for _ in range(2))
    a_side, y = E.fenced_output(c.M, K), E.fenced_output(c.M, rc.width)
    st, _ = _stat_buffer(lib, c.M, rc.G, rc.width, rc.bm)
    native.check(lib.td_conv1x1_fwd_bnrelu(native.ptr(z), native.ptr(w), c.M, rc.G, K, rc.width, native.ptr(part), c.in_rows,
                                           native.ptr(gamma), native.ptr(beta), native.ptr(rm), native.ptr(rv), c.momentum, c.eps,
                                           native.ptr(mean), native.ptr(invstd), native.ptr(a_side.view), native.ptr(y.view),
                                           native.ptr(st.view), native.stream()), "td_conv1x1_fwd_bnrelu")
    torch.cuda.synchronize()
    assert torch.equal(mean.cpu(), c.mean) and torch.equal(invstd.cpu(), torch.ones(rc.G, K))
    _assert_rows(a_side, c.a, "a_side")
    _assert_rows(y, c.y, "y")
    _assert_stats(st, c.stats, "stat_partials")
    assert E.one_ulp(rm.cpu(), c.rm) and E.one_ulp(rv.cpu(), c.rv)


def test_forward_with_batchnorm_relu_prologue(combo):
    _run_bnrelu(E.bnrelu_case(*combo, E.in_rows_for(*combo)))


@pytest.mark.parametrize("in_rows", E.IN_ROWS)
def test_forward_prologue_partial_rows(in_rows):
    _run_bnrelu(E.bnrelu_case("r3", 128, in_rows))            # three groups: every group's rows are shrunk in place


# ---- td_conv1x1_dgrad_bnbwd -----------------------------------------------------------------------------------------------------------

def _run_bnbwd(c, with_res):
    lib, native = _lib()
    rc, Cout = c.rc, c.g.shape[1]
    g, z, w = E.fenced_input(c.g), E.fenced_input(c.z), E.fenced_input(c.w)
    res = E.fenced_input(c.res) if with_res else None
    part = E.fenced_input(c.part.reshape(rc.G * c.in_rows, Cout * 2))
    gamma, beta, mean, invstd = c.gamma.cuda(), c.beta.cuda(), c.mean.cuda(), c.invstd.cuda()
    dgamma, dbeta = (torch.full((Cout,), E.NAN, device="cuda") for _ in range(2))
    dz, dx = E.fenced_output(c.M, Cout), E.fenced_output(c.M, rc.width)
    native.check(lib.td_conv1x1_dgrad_bnbwd(native.ptr(g), native.ptr(z), native.ptr(w), c.M, rc.G, Cout, rc.width, native.ptr(part),
                                            c.in_rows, native.ptr(gamma), native.ptr(beta), native.ptr(mean), native.ptr(invstd),
                                            native.ptr(dgamma), native.ptr(dbeta), native.ptr(dz.view), native.ptr(res), native.ptr(dx.view),
                                            native.stream()), "td_conv1x1_dgrad_bnbwd")
    torch.cuda.synchronize()
    _assert_rows(dz, c.dz, "dz_side")
    _assert_rows(dx, c.dx_res if with_res else c.dx, "dx")
    zero = torch.zeros(Cout)
    assert torch.equal(dgamma.cpu(), zero) and torch.equal(dbeta.cpu(), zero)


@pytest.mark.parametrize("with_res", (False, True))
def test_data_gradient_with_batchnorm_backward_prologue_exact(combo, with_res):
    _run_bnbwd(E.bnbwd_case(*combo, E.in_rows_for(*combo, shift=2)), with_res)


@pytest.mark.parametrize("in_rows", E.IN_ROWS)
def test_data_gradient_prologue_partial_rows(in_rows):
    _run_bnbwd(E.bnbwd_case("r3", 128, in_rows), True)


# ---- td_conv1x1_wgrad, td_conv1x1_wgrad_group -----------------------------------------------------------------------------------------

def _wgrad_ref(r, dt):
    return r.dw.float() if dt == torch.float32 else E.bf(r.dw)


def _wgrad_buffers(lib, r, dt):
    c = r.c
    ws = torch.full((lib.td_conv1x1_wgrad_workspace_floats(c.M, c.K, c.N),), E.NAN, device="cuda")    # slabs that are not launched stay NaN
    assert ws.numel() == c.P * c.N * c.K
    return E.fenced_input(r.dy), E.fenced_input(r.x), E.fenced_output(c.N, c.K, dt), ws


@pytest.mark.parametrize("dt", (torch.float32, torch.bfloat16), ids=("f32", "bf16"))
@pytest.mark.parametrize("i", range(len(E.WGRAD_CASES)))
def test_weight_gradient(i, dt):
    lib, native = _lib()
    r = E.wgrad_case(i)
    c = r.c
    dy, x, dw, ws = _wgrad_buffers(lib, r, dt)
    native.check(lib.td_conv1x1_wgrad(native.ptr(dy), native.ptr(x), c.M, c.K, c.N, c.Hi, c.Wi, c.stride, native.DTYPE_CODES[dt],
                                      native.ptr(dw.view), native.ptr(ws), native.stream()), "td_conv1x1_wgrad")
    torch.cuda.synchronize()
    _assert_rows(dw, _wgrad_ref(r, dt), "dw")


def test_grouped_weight_gradients():
    """One td_conv1x1_wgrad_group call over every case in both dtypes: equal to the single launches bit for bit, hence to the reference."""
    lib, native = _lib()
    probs = [(E.wgrad_case(i), dt) for i in range(len(E.WGRAD_CASES)) for dt in (torch.float32, torch.bfloat16)]
    bufs = [_wgrad_buffers(lib, r, dt) for r, dt in probs]
    single = []
    for (r, dt), (dy, x, _, _) in zip(probs, bufs):
        c = r.c
        _, _, dw, ws = _wgrad_buffers(lib, r, dt)
        native.check(lib.td_conv1x1_wgrad(native.ptr(dy), native.ptr(x), c.M, c.K, c.N, c.Hi, c.Wi, c.stride, native.DTYPE_CODES[dt],
                                          native.ptr(dw.view), native.ptr(ws), native.stream()), "td_conv1x1_wgrad")
        single.append(dw)
    n = len(probs)
    col = lambda name: native.int_array([getattr(r.c, name) for r, _ in probs])
    native.check(lib.td_conv1x1_wgrad_group(n, native.ptr_array([b[0] for b in bufs]), native.ptr_array([b[1] for b in bufs]),
                                            (ctypes.c_longlong * n)(*[r.c.M for r, _ in probs]), col("K"), col("N"), col("Hi"), col("Wi"),
                                            col("stride"), native.int_array([native.DTYPE_CODES[dt] for _, dt in probs]),
                                            native.ptr_array([b[2].view for b in bufs]), native.ptr_array([b[3] for b in bufs]),
                                            native.stream()), "td_conv1x1_wgrad_group")
    torch.cuda.synchronize()
    for (r, dt), b, s in zip(probs, bufs, single):
        E.assert_fence(b[2], "grouped dw")
        assert torch.equal(b[2].view, s.view)
        _assert_rows(s, _wgrad_ref(r, dt), "dw")


# ---- td_conv3x3_fwd, td_conv3x3_wgrad --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(E.CONV3_CASES)))
def test_conv3x3_forward(i):
    lib, native = _lib()
    r = E.conv3_case(i)
    c = r.c
    x, w = E.fenced_input(r.x.reshape(-1, c.Cin)), E.fenced_input(r.w.reshape(c.N, 9 * c.Cin))
    y = E.fenced_output(r.M, c.N)
    st, _ = _stat_buffer(lib, r.M, c.groups, c.N, c.bm)
    native.check(lib.td_conv3x3_fwd(native.ptr(x), native.ptr(w), c.B, c.groups, c.Hi, c.Wi, c.Cin, c.N, c.stride, c.pad, native.ptr(y.view),
                                    native.ptr(st.view), native.stream()), "td_conv3x3_fwd")
    torch.cuda.synchronize()
    _assert_rows(y, r.y, "y")
    _assert_stats(st, r.stats, "stat_partials")


@pytest.mark.parametrize("dt", (torch.float32, torch.bfloat16), ids=("f32", "bf16"))
@pytest.mark.parametrize("pad", (0, 1))
@pytest.mark.parametrize("i", range(len(E.W3_CASES)))
def test_conv3x3_weight_gradient(i, pad, dt):
    lib, native = _lib()
    r = E.w3_case(i, pad)
    c = r.c
    dy, x = E.fenced_input(r.dy.reshape(-1, c.N)), E.fenced_input(r.x.reshape(-1, c.C))
    dw = E.fenced_output(c.N, 9 * c.C, dt)
    ws = torch.full((lib.td_conv3x3_wgrad_workspace_floats(c.B, c.Ho, c.Wo, c.C, c.N),), E.NAN, device="cuda")
    assert ws.numel() == c.P * c.N * 9 * c.C
    native.check(lib.td_conv3x3_wgrad(native.ptr(dy), native.ptr(x), c.B, c.Ho, c.Wo, c.C, c.N, pad, native.DTYPE_CODES[dt],
                                      native.ptr(dw.view), native.ptr(ws), native.stream()), "td_conv3x3_wgrad")
    torch.cuda.synchronize()
    ref = r.dw.reshape(c.N, 9 * c.C)
    _assert_rows(dw, ref.float() if dt == torch.float32 else E.bf(ref), "dw")
