"""The BatchNorm and bias-activation kernels (csrc/td_bn.hip, csrc/td_biasact.hip) through the C ABI on small integer operands, where
every sum they form is exact in any order (tests/bn_exact_util.py: the tiers, the derived bounds, the case tables; their
preconditions and paths are proven in tests/test_bn_exact_cpu.py).  Statistics and dyadic tiers compare with torch.equal (-0 equals
+0); the only tolerances are the two derived bounds of the bounded tier, the ulp count of a multi-group dgamma and the retained
1e-5 sum |gy| of the one leaky-ReLU bias gradient whose terms are not dyadic.

Every operand lies between NaN guard rows, every output (and the workspace) is pre-filled with NaN between guard rows of a marker:
afterwards no NaN is left in an output and no guard row was touched."""
import types

import pytest
import torch

from tests import bn_exact_util as E

pytestmark = pytest.mark.gpu

F32 = torch.float32
DTYPES = pytest.mark.parametrize("dt", (F32, E.BF), ids=("f32", "bf16"))


def _lib():
    import tripled_amd  # noqa: F401
    from tripled_amd import native
    return native.load(), native


def _rows(t, dtype=F32):
    """A host tensor [..., C] as `dtype` rows on the device between NaN guard rows."""
    return E.fenced_input(t.reshape(-1, t.shape[-1]).to(dtype))


def _inout(t):
    f = E.fenced(1, t.numel(), F32, E.MARKER)
    f.view.copy_(t.reshape(1, -1))
    return f


def _workspace(lib, M, G, C):
    n = lib.td_bn_workspace_floats(M, G, C)
    assert n == E.bn_workspace_floats(M, G, C) and n % C == 0
    return E.fenced(n // C, C, F32, E.MARKER)


def _fences(what, *outs, scratch=()):
    for f in outs:
        E.assert_fence(f, what)
    for f in scratch:           # contents undefined (rows that no block owns stay NaN); nothing beyond the stated size is touched
        torch.nan_to_num_(f.view, nan=0.0)
        E.assert_fence(f, what + " workspace")


def _same(f, ref, what):
    got = f.view.cpu()
    assert torch.equal(got, ref.reshape(got.shape).to(got.dtype)), what


def _bounded(f, ref, bnd, what):
    err = (f.view.double().cpu().reshape(ref.shape) - ref).abs()
    print("%s: largest error / bound %.3f" % (what, float((err / bnd.clamp(min=1e-300)).max())))
    assert bool((err <= bnd).all()), what


def _operands(d, G):
    return types.SimpleNamespace(gamma=_rows(d.gamma), beta=_rows(d.beta), rm0=d.rm0, rv0=d.rv0)


# ---- runners: one per family of entry points; every output fenced --------------------------------------------------------------------

def _forward(kind, x, res, dt, p, momentum, eps, relu, M, G, C, part=None, R=0, sums=None, count=None):
    lib, native = _lib()
    o = types.SimpleNamespace(y=E.fenced_output(M, C, dt), mean=E.fenced_output(G, C, F32), invstd=E.fenced_output(G, C, F32),
                              rm=_inout(p.rm0), rv=_inout(p.rv0))
    tail = (p.gamma, p.beta, o.rm.view, o.rv.view, momentum, eps, relu, M, G, C)
    outs = (o.y.view, o.mean.view, o.invstd.view)
    scratch = ()
    if kind == "local":
        scratch = (_workspace(lib, M, G, C),)
        native.call("td_bn_fwd", x, res, dt, *tail, *outs, scratch[0].view)
    elif kind == "partials":
        native.call("td_bn_fwd_from_partials", x, res, dt, *tail, part, R, *outs)
    else:
        native.call("td_bn_sync_fwd_apply", x, res, dt, sums, count, *tail, *outs)
    torch.cuda.synchronize()
    _fences(kind + " forward", o.y, o.mean, o.invstd, o.rm, o.rv, scratch=scratch)
    return o


def _backward(kind, dy, x, y, dt, p, mean, invstd, relu, with_res, M, G, C, part=None, R=0, local=None, glob=None, count=None):
    lib, native = _lib()
    o = types.SimpleNamespace(dx=E.fenced_output(M, C, dt), dres=E.fenced_output(M, C, dt) if with_res else None,
                              dgamma=E.fenced_output(1, C, F32), dbeta=E.fenced_output(1, C, F32))
    dres = o.dres.view if with_res else None
    mid = (p.gamma, p.beta, mean, invstd, relu, M, G, C)
    scratch = ()
    if kind == "local":
        scratch = (_workspace(lib, M, G, C),)
        native.call("td_bn_bwd", dy, x, y, dt, *mid, o.dx.view, dres, o.dgamma.view, o.dbeta.view, scratch[0].view)
    elif kind == "partials":
        native.call("td_bn_bwd_from_partials", dy, x, y, dt, *mid, part, R, o.dx.view, dres, o.dgamma.view, o.dbeta.view)
    else:
        coef = E.fenced_output(G, 3 * C, F32)
        native.call("td_bn_sync_bwd_dx", dy, x, y, dt, local, glob, count, *mid, o.dx.view, dres, o.dgamma.view, o.dbeta.view, coef.view)
        E.assert_fence(coef, "coef")
    torch.cuda.synchronize()
    _fences(kind + " backward", *(f for f in (o.dx, o.dres, o.dgamma, o.dbeta) if f is not None), scratch=scratch)
    return o


def _check_stats(o, st, what):
    _same(o.mean, st.mean, what + " save_mean")
    _same(o.invstd, st.invstd, what + " save_invstd")
    _same(o.rm, st.rm, what + " running_mean")
    _same(o.rv, st.rv, what + " running_var")


def _check_param_grads(o, ref, G, what):
    _same(o.dbeta, ref.dbeta, what + " dbeta")
    got = o.dgamma.view.cpu().reshape(-1)
    assert E.within_ulps(got, ref.dgamma, G - 1), what + " dgamma"        # G = 1: the float32 product, bit for bit


def _momentum(relu, with_res):
    return E.MOMENTUM_TENTH if (relu, with_res) == (1, True) else 0.25


# ---- the replicas of the cut functions against the library ---------------------------------------------------------------------------

def test_cut_replicas_agree_with_the_library():
    lib, _ = _lib()
    for c in E.BN_CASES:
        M = c.Mg * c.G
        assert lib.td_bn_partial_rows(M, c.G, c.C) == E.bn_cut(c.Mg, c.C, stat=True).S_eff == E.STAT_ROWS[c.id]
        assert lib.td_bn_workspace_floats(M, c.G, c.C) == E.bn_workspace_floats(M, c.G, c.C)
    for c in E.BA_CASES:
        assert lib.td_bias_act_workspace_floats(c.M, c.C) == E.ba_workspace_floats(c.M, c.C) == c.blocks * c.C


# ---- td_bn_fwd, td_bn_bwd --------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("cid", E.GENERAL_IDS)
def test_general_data_statistics_exact_outputs_bounded(cid, dt):
    d = E.general_case(cid)
    c, p = d.c, _operands(d, d.c.G)
    x, res, xb, dy = _rows(d.x, dt), _rows(d.res, dt), _rows(d.xb, dt), _rows(d.dy, dt)
    meanb, invstdb = _rows(d.meanb), _rows(d.invstdb)
    for relu, with_res in E.VARIANTS:
        what = "%s relu %d residual %d" % (cid, relu, with_res)
        momentum = _momentum(relu, with_res)
        st, y, bnd = E.general_forward(cid, relu, with_res, momentum, dt)
        o = _forward("local", x, res if with_res else None, dt, p, momentum, E.EPS, relu, d.M, c.G, c.C)
        _check_stats(o, st, what)
        _bounded(o.y, y, bnd, what + " y")
        r = E.general_backward(cid, relu, with_res, dt)
        y_in = _rows(r.y_in, dt) if relu else None
        b = _backward("local", dy, xb, y_in, dt, p, meanb, invstdb, relu, with_res, d.M, c.G, c.C)
        _check_param_grads(b, r, c.G, what)
        if with_res:
            _same(b.dres, r.gm, what + " dres")
        _bounded(b.dx, r.dx, r.bound, what + " dx")


def _dyadic_forward_backward(kind, d, dt, G, C, variants, **kw):
    """Forward and backward of dyadic data through one family of entry points: every output bit for bit."""
    p = _operands(d, G)
    x, res = _rows(d.x, dt), _rows(d.res, dt)
    mean, invstd = _rows(d.mean), _rows(d.invstd)
    for relu, with_res in variants:
        what = "%s relu %d residual %d" % (kind, relu, with_res)
        v = d.variants[(relu, with_res)]
        momentum = _momentum(relu, with_res)
        o = _forward(kind, x, res if with_res else None, dt, p, momentum, E.EPS_DYADIC, relu, d.M, G, C, **kw.get("fwd", lambda: {})())
        _check_stats(o, E.dyadic_stats(d, momentum, kw.get("count_factor", 1)), what)
        _same(o.y, v.y, what + " y")
        dy = _rows(v.dy, dt)
        for from_x in ((False, True) if relu and not with_res else (False,)):       # the mask read from y / recomputed from x
            b = _backward(kind, dy, x, None if from_x or not relu else o.y.view, dt, p, mean, invstd, relu, with_res, d.M, G, C,
                          **kw.get("bwd", lambda v: {})(v))
            w = what + (" mask from x" if from_x else "")
            _check_param_grads(b, v, 1, w)                   # invstd = 0.5: the ordered float32 sum is exact, whatever G is
            _same(b.dx, v.dx, w + " dx")
            if with_res:
                _same(b.dres, v.gm, w + " dres")


@DTYPES
@pytest.mark.parametrize("cid", E.DYADIC_IDS)
def test_dyadic_data_every_output_exact(cid, dt):
    d = E.dyadic_case(cid)
    _dyadic_forward_backward("local", d, dt, d.c.G, d.c.C, E.VARIANTS)


# ---- td_bn_fwd_partials, td_bn_bwd_partials ----------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("cid", [c.id for c in E.BN_CASES])
def test_partial_rows_are_the_sums_of_their_splits(cid, dt):
    lib, native = _lib()
    c = E.BN[cid]
    M, rows = c.Mg * c.G, E.STAT_ROWS[cid]
    general = cid in E.GENERAL_IDS and c.Mg % 2
    d = E.general_case(cid) if general else E.dyadic_case(cid)
    p = _operands(d, c.G)
    x = _rows(d.x, dt)
    out = E.fenced_output(c.G * rows, 2 * c.C, F32)
    native.call("td_bn_fwd_partials", x, dt, M, c.G, c.C, out.view)
    torch.cuda.synchronize()
    E.assert_fence(out, "forward partial rows")
    _same(out, d.part_stat.float(), cid + " forward partial rows")
    xb, mean, invstd = (_rows(d.xb, dt), _rows(d.meanb), _rows(d.invstdb)) if general else (x, _rows(d.mean), _rows(d.invstd))
    for relu, from_x in ((0, False), (1, False)) + (() if general else ((1, True),)):
        if general:
            r = E.general_backward(cid, relu, False, dt, stat=True)
            dy, y_in, ref = d.dy, r.y_in, r.part
        else:
            v = d.variants[(relu, False)]
            dy, y_in, ref = v.dy, E.stored(v.y, dt), E.backward_partials(d, v, stat=True)
        y = None if from_x or not relu else _rows(y_in, dt)
        out = E.fenced_output(c.G * rows, 2 * c.C, F32)
        native.call("td_bn_bwd_partials", _rows(dy, dt), xb, y, dt, p.gamma, p.beta, mean, invstd, relu, M, c.G, c.C, out.view)
        torch.cuda.synchronize()
        E.assert_fence(out, "backward partial rows")
        _same(out, ref.float(), "%s backward partial rows relu %d from x %d" % (cid, relu, from_x))


# ---- td_bn_fwd_from_partials, td_bn_bwd_from_partials --------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("i", range(len(E.PART_CASES)), ids=[str(pc.R) for pc in E.PART_CASES])
def test_caller_made_partial_rows(i, dt):
    """The partial rows are scratch (more than 96 are reduced in place): a fresh copy for every call."""
    d = E.partials_case(i)
    pc = d.pc
    flat = lambda t: t.reshape(pc.G * pc.R, 2 * E.PART_C)
    _dyadic_forward_backward("partials", d, dt, pc.G, E.PART_C, E.VARIANTS,
                             fwd=lambda: dict(part=E.fenced_input(flat(d.part_fwd)), R=pc.R),
                             bwd=lambda v: dict(part=E.fenced_input(flat(d.part_bwd)), R=pc.R))


# ---- td_bn_sync_fwd_sums, td_bn_sync_fwd_apply, td_bn_sync_bwd_sums, td_bn_sync_bwd_dx: one process, no process group ------------------

def _sync_sums(name, args, M, G, C):
    lib, native = _lib()
    sums, ws = E.fenced_output(G, 2 * C, F32), _workspace(lib, M, G, C)
    native.call(name, *args, M, G, C, sums.view, ws.view)
    torch.cuda.synchronize()
    _fences(name, sums, scratch=(ws,))
    return sums


def _equal_outputs(a, b, names, what):
    for n in names:
        fa, fb = getattr(a, n), getattr(b, n)
        assert (fa is None) == (fb is None)
        if fa is not None:
            assert torch.equal(fa.view, fb.view), "%s: %s differs from the local form" % (what, n)


@DTYPES
@pytest.mark.parametrize("cid", [c.id for c in E.BN_CASES])
def test_synchronised_entry_points_in_one_process(cid, dt):
    """(1) the local sums are exact; (2) with global = local sums and count = Mg every output equals td_bn_fwd / td_bn_bwd bit for
    bit; (3) with twice the sums over twice the rows -- two ranks with equal data -- the outputs match the float64 replica (the
    statistics exactly; the unbiased variance is over 2 Mg rows), dgamma / dbeta coming from the local sums only."""
    c = E.BN[cid]
    M, G, C = c.Mg * c.G, c.G, c.C
    general = cid in E.GENERAL_IDS and c.Mg % 2
    d = E.general_case(cid) if general else E.dyadic_case(cid)
    p = _operands(d, G)
    eps = E.EPS if general else E.EPS_DYADIC
    x, res = _rows(d.x, dt), _rows(d.res, dt)
    sums = _sync_sums("td_bn_sync_fwd_sums", (x, dt), M, G, C)
    _same(sums, torch.stack([d.A, d.B], -1).float(), cid + " local forward sums")
    count = [torch.full((1,), float(k * c.Mg), device="cuda") for k in (1, 2)]
    twice = 2 * sums.view
    xb, mean, invstd = (_rows(d.xb, dt), _rows(d.meanb), _rows(d.invstdb)) if general else (x, _rows(d.mean), _rows(d.invstd))
    for relu, with_res in E.VARIANTS:
        what = "%s relu %d residual %d" % (cid, relu, with_res)
        momentum = _momentum(relu, with_res)
        r_ = res if with_res else None
        local = _forward("local", x, r_, dt, p, momentum, eps, relu, M, G, C)
        one = _forward("sync", x, r_, dt, p, momentum, eps, relu, M, G, C, sums=sums.view, count=count[0])
        _equal_outputs(one, local, ("y", "mean", "invstd", "rm", "rv"), what)
        two = _forward("sync", x, r_, dt, p, momentum, eps, relu, M, G, C, sums=twice, count=count[1])
        if general:
            st, y, bnd = E.general_forward(cid, relu, with_res, momentum, dt, count_factor=2)
            _bounded(two.y, y, bnd, what + " y of two ranks")
            r = E.general_backward(cid, relu, with_res, dt, count_factor=2)
            dy, y_in = _rows(d.dy, dt), (_rows(r.y_in, dt) if relu else None)
        else:
            st, r = E.dyadic_stats(d, momentum, 2), d.variants[(relu, with_res)]
            _same(two.y, r.y, what + " y of two ranks")
            dy, y_in = _rows(r.dy, dt), (_rows(E.stored(r.y, dt), dt) if relu else None)
        _check_stats(two, st, what + " two ranks")
        bsums = _sync_sums("td_bn_sync_bwd_sums", (dy, xb, y_in, dt, p.gamma, p.beta, mean, invstd, relu), M, G, C)
        _same(bsums, torch.stack([r.A, r.B], -1).float(), what + " local backward sums")
        blocal = _backward("local", dy, xb, y_in, dt, p, mean, invstd, relu, with_res, M, G, C)
        bone = _backward("sync", dy, xb, y_in, dt, p, mean, invstd, relu, with_res, M, G, C, local=bsums.view, glob=bsums.view, count=count[0])
        _equal_outputs(bone, blocal, ("dx", "dres", "dgamma", "dbeta"), what)
        btwo = _backward("sync", dy, xb, y_in, dt, p, mean, invstd, relu, with_res, M, G, C, local=bsums.view, glob=2 * bsums.view,
                         count=count[1])
        _check_param_grads(btwo, r, G if general else 1, what + " two ranks")
        if with_res:
            _same(btwo.dres, r.gm, what + " dres of two ranks")
        if general:
            _bounded(btwo.dx, r.dx, r.bound, what + " dx of two ranks")
        else:
            _same(btwo.dx, r.dx, what + " dx of two ranks")


# ---- td_bias_act_fwd, td_bias_act_bwd -------------------------------------------------------------------------------------------------------

def _bias_act_backward(r, dt, db_dt):
    lib, native = _lib()
    M, C = r.M, r.C
    up, a = _rows(r.up, dt), (_rows(E.stored(r.a, dt), dt) if r.act else None)
    gy, db = E.fenced_output(M, C, dt), E.fenced_output(1, C, db_dt)
    ws = E.fenced_output(E.ba_blocks(M * (C // 8)), C, F32)
    native.call("td_bias_act_bwd", up, a, dt, M, C, r.act, gy.view, db.view, db_dt, ws.view)
    torch.cuda.synchronize()
    _fences("td_bias_act_bwd", db, ws)                      # every block writes its row of the workspace
    if r.act == 0:                                          # gy is not written
        assert bool(torch.isnan(gy.view).all())
        gy.view.zero_()
    E.assert_fence(gy, "gy")
    return gy, db


def _check_bias_act(r, dt):
    lib, native = _lib()
    M, C = r.M, r.C
    what = "%d x %d act %d" % (M, C, r.act)
    if r.fwd is not None:           # ELU's forward stays with tests/test_hip_biasact.py: expm1f is not replicable
        a = E.fenced_output(M, C, dt)
        native.call("td_bias_act_fwd", _rows(r.y, dt), _rows(r.bias, dt), dt, dt, M, C, r.act, a.view)      # the bias in the tensors' dtype
        torch.cuda.synchronize()
        E.assert_fence(a, what + " forward")
        _same(a, E.stored(r.fwd, dt), what + " forward")
    (gy, db), (gy2, db2) = _bias_act_backward(r, dt, F32), _bias_act_backward(r, dt, F32)
    assert torch.equal(gy.view, gy2.view) and torch.equal(db.view, db2.view), what + ": two runs differ"
    if r.act:
        _same(gy, E.stored(r.gy, dt), what + " gy")
    _, dbb = _bias_act_backward(r, dt, E.BF)
    if r.exact:
        _same(db, r.dbias.float(), what + " dbias")
        _same(dbb, E.bf(r.dbias), what + " dbias in bf16")
    else:                           # the retained tolerance of tests/test_hip_biasact.py: a float32 sum of terms that are not dyadic
        err = float((db.view.double().cpu().reshape(-1) - r.dbias).abs().max())
        print("%s: dbias error %.3g of sum |gy| %.3g" % (what, err, r.abs_sum))
        assert err <= 1e-5 * r.abs_sum
        assert torch.equal(dbb.view.cpu().reshape(-1), db.view.cpu().reshape(-1).to(E.BF))


@DTYPES
@pytest.mark.parametrize("act", E.ACTS)
@pytest.mark.parametrize("c", E.BA_CASES, ids=["%dx%d" % c[:2] for c in E.BA_CASES])
def test_bias_act_exact(c, act, dt):
    _check_bias_act(E.ba_case(c.M, c.C, act), dt)


@DTYPES
def test_leaky_relu_with_gradients_under_the_slope(dt):
    _check_bias_act(E.ba_case(32769, 8, 2, True), dt)
