"""The host layer under the BatchNorm, 1x1 GEMM, join, max-pool and l1-map entry points, on a host WITHOUT a device.

Three things are pinned, all without a kernel ever running:
  * the return code of every argument check, and the ORDER of the checks (a table of literal cases; every case returns before any HIP
    call, so the table describes any build of the ABI: TD_HIP_LIB selects another one);
  * that every launch status is recorded under the name of the entry point that was called (td_last_hip_error);
  * that native.check quotes that record only for TD_ERR_LAUNCH.

The module hands HOST buffers to the library as pointers, so it must never run where a launch could succeed: it skips as a whole,
before the library is loaded, unless torch.cuda.is_available() is false.
"""
import ctypes

import pytest
import torch

if torch.cuda.is_available():
    pytest.skip("host buffers are passed as pointers: only where no launch can succeed", allow_module_level=True)

import tripled_amd  # noqa: E402,F401
from tripled_amd import native  # noqa: E402

BAD, UNS, LAUNCH = -1, -2, -3
_BUF = ctypes.create_string_buffer(1 << 16)
P = ctypes.cast(_BUF, ctypes.c_void_p).value      # a non-null pointer (host memory: never dereferenced, no launch succeeds here)
FOUR = (ctypes.c_longlong * 4)(1, 1, 1, 1)
BIG = 1 << 34                                      # rows: BIG * 64 = 2^40 elements


@pytest.fixture(scope="module")
def lib():
    return native.load()


# ---- valid calls: name -> arguments in the header's order (without the stream) --------------------------------------------------
_SHAPE = dict(M=128, groups=1, C=64)
_BWD_IN = dict(dy=P, x=P, y=P, dtype=1, gamma=P, beta=P, save_mean=P, save_invstd=P, relu=1)
_FWD_IN = dict(x=P, residual=None, dtype=1, gamma=P, beta=P, running_mean=P, running_var=P, momentum=0.1, eps=1e-5, relu=1)
_DX_OUT = dict(dx=P, dresidual=None, dgamma=P, dbeta=P)
_POOL = dict(dtype=1, N=1, H=8, W=8, C=8)
VALID = {
    "td_bn_fwd": dict(_FWD_IN, **_SHAPE, y=P, out_mean=P, out_invstd=P, workspace=P),
    "td_bn_bwd": dict(_BWD_IN, **_SHAPE, **_DX_OUT, workspace=P),
    "td_bn_fwd_from_partials": dict(_FWD_IN, **_SHAPE, partials=P, stat_rows=2, y=P, out_mean=P, out_invstd=P),
    "td_bn_fwd_partials": dict(x=P, dtype=1, **_SHAPE, partials=P),
    "td_bn_bwd_partials": dict(_BWD_IN, **_SHAPE, partials=P),
    "td_bn_bwd_from_partials": dict(_BWD_IN, **_SHAPE, partials=P, stat_rows=2, **_DX_OUT),
    "td_bn_sync_fwd_sums": dict(x=P, dtype=1, **_SHAPE, sums=P, workspace=P),
    "td_bn_sync_fwd_apply": dict(x=P, residual=None, dtype=1, sums=P, count=P, gamma=P, beta=P, running_mean=P, running_var=P,
                                 momentum=0.1, eps=1e-5, relu=1, **_SHAPE, y=P, out_mean=P, out_invstd=P),
    "td_bn_sync_bwd_sums": dict(_BWD_IN, **_SHAPE, sums=P, workspace=P),
    "td_bn_sync_bwd_dx": dict(dy=P, x=P, y=P, dtype=1, local_sums=P, global_sums=P, count=P, gamma=P, beta=P, save_mean=P,
                              save_invstd=P, relu=1, **_SHAPE, **_DX_OUT, coef=P),
    "td_conv1x1_fwd": dict(x=P, w=P, M=128, groups=1, K=64, N=64, Hi=0, Wi=0, stride=1, y=P, stat_partials=None),
    "td_conv1x1_wgrad": dict(dy=P, x=P, M=128, K=64, N=64, Hi=0, Wi=0, stride=1, dw_dtype=1, dw=P, workspace=P),
    "td_join_fwd": dict(a=P, b=P, tail=P, dtype=1, npix=16, C0=8, C1=8, C2=1, out=P),
    "td_join_bwd": dict(grad_out=P, dtype=1, npix=16, C0=8, C1=8, C2=1, grad_a=P, grad_b=P, grad_tail=P),
    "td_join_up2_fwd": dict(a=P, b_half=P, tail=P, dtype=1, N=1, H=4, W=4, C0=8, C1=8, C2=1, out=P),
    "td_join_up2_bwd": dict(grad_out=P, dtype=1, N=1, H=4, W=4, C0=8, C1=8, C2=1, grad_a=P, grad_b_half=P, grad_tail=P),
    "td_maxpool5_fwd": dict(inp=P, **_POOL, out=P, idx=P),
    "td_maxpool5_bwd": dict(grad_out=P, idx=P, **_POOL, grad_in=P),
    "td_maxpool5_bwd_add": dict(grad_out=P, idx=P, add=None, **_POOL, grad_in=P),
    "td_maxpool3s2_fwd": dict(inp=P, **_POOL, out=P, idx=P),
    "td_maxpool3s2_bwd": dict(grad_out=P, idx=P, **_POOL, grad_in=P),
    "td_l1map_fwd": dict(pred=P, dtype=1, strides=FOUR, target=P, B=1, C=3, H=8, W=8, weight=1.0, out=P),
    "td_l1map_bwd": dict(pred=P, dtype=1, strides=FOUR, target=P, gmap=P, B=1, C=3, H=8, W=8, weight=1.0, dpred=P),
    # reached by the launch-status test only
    "td_conv1x1_fwd_bnrelu": dict(z=P, w=P, M=128, groups=1, K=64, N=64, in_partials=P, in_rows=2, gamma=P, beta=P, running_mean=None,
                                  running_var=None, momentum=0.1, eps=1e-5, save_mean=P, save_invstd=P, a_side=None, y=P,
                                  stat_partials=None),
    "td_conv1x1_fwd_sum": dict(x=P, w=P, M=128, K=64, N=64, run_in=P, y=P, run_out=P),
    "td_conv1x1_dgrad": dict(dy=P, w=P, M=128, groups=1, Cout=64, Cin=64, residual=None, dx=P),
    "td_conv1x1_dgrad_bnsums": dict(dy=P, w=P, M=128, groups=1, Cout=64, Cin=64, z=P, gamma=P, beta=P, save_mean=P, save_invstd=P,
                                    dx=P, out_partials=P),
    "td_conv1x1_dgrad_bnbwd": dict(g=P, z=P, w=P, M=128, groups=1, Cout=64, Cin=64, in_partials=P, in_rows=2, gamma=P, beta=P,
                                   save_mean=P, save_invstd=P, dgamma=P, dbeta=P, dz_side=None, residual=None, dx=P),
    "td_conv3x3_fwd": dict(x=P, w=P, B=1, groups=1, Hi=8, Wi=8, Cin=64, N=64, stride=1, pad=1, y=P, stat_partials=None),
    "td_conv3x3_wgrad": dict(dy=P, x=P, B=1, Ho=8, Wo=32, C=64, N=64, pad=1, dw_dtype=1, dw=P, workspace=P),
}


def call(lib, name, **changes):
    args = dict(VALID[name])
    assert set(changes) <= set(args), (name, set(changes) - set(args))
    args.update(changes)
    assert len(args) == len(native.SIGNATURES[name][1]) - 1, name
    return getattr(lib, name)(*args.values(), None)


def group_call(lib, problems, n=None, **nulls):
    """td_conv1x1_wgrad_group over `problems` (each: changes to the valid td_conv1x1_wgrad call)."""
    rows = [dict(VALID["td_conv1x1_wgrad"], **p) for p in problems]
    col = lambda key: [r[key] for r in rows]
    ptrs = lambda key: (ctypes.c_void_p * len(rows))(*col(key))
    ints = lambda key: (ctypes.c_int * len(rows))(*col(key))
    args = dict(dy=ptrs("dy"), x=ptrs("x"), M=(ctypes.c_longlong * len(rows))(*col("M")), K=ints("K"), N=ints("N"), Hi=ints("Hi"),
                Wi=ints("Wi"), stride=ints("stride"), dw_dtype=ints("dw_dtype"), dw=ptrs("dw"), workspace=ptrs("workspace"))
    args.update(nulls)
    return lib.td_conv1x1_wgrad_group(len(rows) if n is None else n, *args.values(), None)


# ---- the return-code table ------------------------------------------------------------------------------------------------------
BN = [n for n in VALID if n.startswith("td_bn_")]
BN_REQUIRED = {
    "td_bn_fwd": ["x", "gamma", "beta", "y", "out_mean", "out_invstd", "workspace"],
    "td_bn_bwd": ["dy", "x", "gamma", "save_mean", "save_invstd", "dx", "dgamma", "dbeta", "workspace"],
    "td_bn_fwd_from_partials": ["x", "gamma", "beta", "y", "out_mean", "out_invstd", "partials"],
    "td_bn_fwd_partials": ["x", "partials"],
    "td_bn_bwd_partials": ["dy", "x", "gamma", "save_mean", "save_invstd", "partials"],
    "td_bn_bwd_from_partials": ["dy", "x", "gamma", "save_mean", "save_invstd", "dx", "dgamma", "dbeta", "partials"],
    "td_bn_sync_fwd_sums": ["x", "sums", "workspace"],
    "td_bn_sync_fwd_apply": ["x", "sums", "count", "gamma", "beta", "y", "out_mean", "out_invstd"],
    "td_bn_sync_bwd_sums": ["dy", "x", "gamma", "save_mean", "save_invstd", "sums", "workspace"],
    "td_bn_sync_bwd_dx": ["dy", "x", "local_sums", "global_sums", "count", "gamma", "save_mean", "save_invstd", "dx", "dgamma", "dbeta",
                          "coef"],
}
BN_MASK = ["td_bn_bwd", "td_bn_bwd_partials", "td_bn_bwd_from_partials", "td_bn_sync_bwd_sums", "td_bn_sync_bwd_dx"]      # relu && !y
BN_DRES = ["td_bn_bwd", "td_bn_bwd_from_partials", "td_bn_sync_bwd_dx"]
BN_RUNNING = ["td_bn_fwd", "td_bn_fwd_from_partials", "td_bn_sync_fwd_apply"]

TABLE = []
for _n in BN:
    TABLE += [(_n, {p: None}, BAD) for p in BN_REQUIRED[_n]]
    TABLE += [(_n, dict(M=0), BAD), (_n, dict(M=-128), BAD), (_n, dict(C=0), BAD), (_n, dict(M=129, groups=2), BAD),
              (_n, dict(groups=0), BAD), (_n, dict(M=65 * 64, groups=65), BAD), (_n, dict(M=64 * 64, groups=64, C=32), UNS),
              (_n, dict(C=32), UNS), (_n, dict(C=96), UNS), (_n, dict(M=BIG), UNS), (_n, dict(M=BIG // 2, C=128), UNS),
              (_n, dict(dtype=7), UNS), (_n, dict(dtype=-1), UNS),
              (_n, {BN_REQUIRED[_n][-1]: None, "C": 32}, BAD),          # order: a null pointer before the channel limit
              (_n, {BN_REQUIRED[_n][0]: None, "dtype": 7}, BAD),
              (_n, dict(M=129, groups=2, C=32), BAD), (_n, dict(C=32, dtype=7), UNS)]
for _n in BN_RUNNING:
    TABLE += [(_n, dict(running_var=None), BAD), (_n, dict(running_mean=None), BAD), (_n, dict(running_mean=None, C=32), BAD),
              (_n, dict(running_mean=None, running_var=None, C=32), UNS)]
for _n in BN_MASK:
    TABLE += [(_n, dict(relu=2), BAD), (_n, dict(relu=-1), BAD), (_n, dict(relu=2, C=32), BAD),
              (_n, dict(y=None, beta=None), BAD), (_n, dict(y=None, beta=None, C=32), BAD),
              (_n, dict(y=None, C=32), UNS),                            # the mask from x is allowed: the channel limit decides
              (_n, dict(relu=0, y=None, beta=None, C=32), UNS)]
for _n in BN_DRES:
    TABLE += [(_n, dict(y=None, dresidual=P), BAD), (_n, dict(y=None, dresidual=P, C=32), BAD), (_n, dict(dresidual=P, C=32), UNS),
              (_n, dict(relu=0, y=None, dresidual=P, dtype=7), UNS)]
for _n in ("td_bn_fwd_from_partials", "td_bn_bwd_from_partials"):
    TABLE += [(_n, dict(stat_rows=0), BAD), (_n, dict(stat_rows=-3), BAD), (_n, dict(stat_rows=0, C=32), BAD)]

_n = "td_conv1x1_fwd"
TABLE += [(_n, dict(x=None), BAD), (_n, dict(w=None), BAD), (_n, dict(y=None), BAD), (_n, dict(M=0), BAD), (_n, dict(M=129, groups=2), BAD),
          (_n, dict(groups=0), BAD), (_n, dict(M=65 * 64, groups=65), BAD), (_n, dict(K=32), BAD), (_n, dict(N=96), BAD), (_n, dict(K=0), BAD),
          (_n, dict(stride=0), BAD), (_n, dict(stride=2, Hi=0, Wi=8), BAD), (_n, dict(stride=2, Hi=8, Wi=0), BAD),
          (_n, dict(stride=2, Hi=8, Wi=8, M=24), BAD),                  # Ho Wo = 16 does not divide M
          (_n, dict(M=BIG), UNS), (_n, dict(M=BIG // 2, N=128), UNS), (_n, dict(M=BIG, y=None), BAD), (_n, dict(M=BIG, stride=2), BAD)]
_n = "td_conv1x1_wgrad"
WGRAD_CASES = [(dict(M=0), BAD), (dict(K=32), BAD), (dict(N=0), BAD), (dict(stride=0), BAD), (dict(dw_dtype=7), UNS),
               (dict(dw_dtype=7, stride=2, Hi=0), UNS),                  # the dtype is checked before the geometry
               (dict(dw_dtype=7, stride=0), BAD), (dict(stride=2, Hi=0, Wi=8), BAD), (dict(stride=2, Hi=8, Wi=0), BAD),
               (dict(stride=2, Hi=8, Wi=8, M=24), BAD), (dict(M=BIG), UNS), (dict(M=BIG // 2, K=128), UNS), (dict(M=BIG, dw_dtype=7), UNS)]
TABLE += [(_n, c, code) for c, code in WGRAD_CASES]
TABLE += [(_n, dict(dy=None), BAD), (_n, dict(x=None), BAD), (_n, dict(dw=None), BAD), (_n, dict(workspace=None), BAD),
          (_n, dict(dw=None, dw_dtype=7), BAD), (_n, dict(workspace=None, M=BIG), BAD)]
for _n in ("td_join_fwd", "td_join_bwd", "td_join_up2_fwd", "td_join_up2_bwd"):
    _ptrs = [k for k, v in VALID[_n].items() if v == P]
    _rows = "npix" if "npix" in VALID[_n] else "N"
    TABLE += [(_n, {p: None}, BAD) for p in _ptrs]
    TABLE += [(_n, {_rows: 0}, BAD), (_n, dict(C0=0), BAD), (_n, dict(C1=-8), BAD), (_n, dict(C2=0), BAD), (_n, dict(C0=4), UNS),
              (_n, dict(C1=12), UNS), (_n, dict(C2=9), UNS), (_n, dict(dtype=7), UNS), (_n, {_ptrs[0]: None, "C0": 4}, BAD),
              (_n, {_ptrs[-1]: None, "dtype": 7}, BAD), (_n, dict(C0=4, dtype=7), UNS)]
TABLE += [("td_join_fwd", dict(npix=1 << 36), UNS), ("td_join_bwd", dict(npix=1 << 36), UNS),
          ("td_join_up2_fwd", dict(H=3), UNS), ("td_join_up2_fwd", dict(W=6, H=5), UNS), ("td_join_up2_bwd", dict(W=3), UNS),
          ("td_join_up2_fwd", dict(H=0), BAD), ("td_join_up2_bwd", dict(W=0), BAD),
          ("td_join_up2_fwd", dict(N=1 << 16, H=1 << 10, W=1 << 10), UNS), ("td_join_up2_bwd", dict(N=1 << 16, H=1 << 10, W=1 << 10), UNS)]
for _n in ("td_maxpool5_fwd", "td_maxpool5_bwd", "td_maxpool5_bwd_add", "td_maxpool3s2_fwd", "td_maxpool3s2_bwd"):
    _ptrs = [k for k, v in VALID[_n].items() if v == P]
    TABLE += [(_n, {p: None}, BAD) for p in _ptrs]
    TABLE += [(_n, dict(N=0), BAD), (_n, dict(H=0), BAD), (_n, dict(W=-1), BAD), (_n, dict(C=0), BAD), (_n, dict(C=4), UNS),
              (_n, dict(C=12), UNS), (_n, dict(dtype=7), UNS), (_n, {_ptrs[0]: None, "C": 4}, BAD), (_n, {_ptrs[-1]: None, "dtype": 7}, BAD)]
for _n, _outs in (("td_l1map_fwd", ["out"]), ("td_l1map_bwd", ["gmap", "dpred"])):
    TABLE += [(_n, dict(pred=None), BAD), (_n, dict(target=None), BAD), (_n, dict(strides=None), BAD), (_n, dict(B=0), BAD),
              (_n, dict(C=0), BAD), (_n, dict(H=0), BAD), (_n, dict(W=0), BAD), (_n, dict(C=65), UNS),
              (_n, dict(B=1 << 10, C=64, H=1 << 12, W=1 << 12), UNS), (_n, dict(dtype=7), UNS), (_n, dict(pred=None, C=65), BAD)]
    TABLE += [(_n, {o: None}, BAD) for o in _outs]
    TABLE += [(_n, {_outs[-1]: None, "C": 65}, UNS),                     # the shared shape check comes before the entry point's own pointers
              (_n, {_outs[-1]: None, "dtype": 7}, BAD)]


def _case_id(case):
    name, changes, code = case
    return "%s-%s-%d" % (name, ",".join("%s=%s" % (k, "P" if v == P else v) for k, v in changes.items()), code)


def test_table_covers_every_touched_entry_point():
    covered = {name for name, _, _ in TABLE}
    assert covered == {n for n in VALID if n.startswith(("td_bn_", "td_join_", "td_maxpool", "td_l1map_"))} | {"td_conv1x1_fwd", "td_conv1x1_wgrad"}
    assert len(BN) == 10 and len(TABLE) > 400      # td_bn_fwd_partials ... td_bn_sync_bwd_dx: the launching BatchNorm entry points


@pytest.mark.parametrize("case", TABLE, ids=_case_id)
def test_return_code(lib, case):
    name, changes, code = case
    assert call(lib, name, **changes) == code


GOOD = {}
GROUP_TABLE = [([GOOD], dict(n=-1), BAD), ([GOOD], dict(dy=None), BAD), ([GOOD], dict(M=None), BAD), ([GOOD], dict(workspace=None), BAD),
               ([GOOD, dict(dy=None)], {}, BAD), ([GOOD, GOOD, dict(workspace=None)], {}, BAD)]
GROUP_TABLE += [([GOOD, c], {}, code) for c, code in WGRAD_CASES if not ("M" in c and c["M"] >= BIG // 2 and "stride" in c)]
GROUP_TABLE += [([GOOD, dict(dw_dtype=7), dict(stride=2, Hi=0)], {}, UNS),       # the first failing problem decides
                ([GOOD, dict(stride=2, Hi=0), dict(dw_dtype=7)], {}, BAD),
                ([dict(M=BIG), dict(K=32)], {}, UNS), ([dict(dw=None, dw_dtype=7), GOOD], {}, BAD),
                ([GOOD] * 4097, {}, UNS), ([GOOD] * 4096 + [dict(K=32)], {}, BAD)]


@pytest.mark.parametrize("case", GROUP_TABLE, ids=lambda c: "%dx-%s-%s-%d" % (len(c[0]), c[0][-1] if len(c[0]) < 9 else "", c[1], c[2]))
def test_group_return_code(lib, case):
    problems, extra, code = case
    assert group_call(lib, problems, **extra) == code


# ---- launch status --------------------------------------------------------------------------------------------------------------
# a valid call per entry point, ordered so that the failure before each one belongs to ANOTHER entry point: all seventeen status
# returns of td_bn (8), td_conv1x1 (4: the GEMM launcher, the slab sum, the single and the grouped weight gradient), td_join (2),
# td_conv3x3 and td_conv3x3_wgrad
LAUNCHES = BN + ["td_conv1x1_fwd", "td_conv1x1_fwd_bnrelu", "td_conv1x1_fwd_sum", "td_conv1x1_dgrad", "td_conv1x1_dgrad_bnsums",
                 "td_conv1x1_dgrad_bnbwd", "td_conv1x1_wgrad", "td_conv1x1_wgrad_group", "td_join_fwd", "td_join_bwd", "td_join_up2_fwd",
                 "td_join_up2_bwd", "td_conv3x3_fwd", "td_conv3x3_wgrad"]


def test_launch_failure_names_the_entry_point_called(lib):
    assert len(set(LAUNCHES)) == len(LAUNCHES) == 24
    assert lib.td_bias_act_fwd(P, P, 0, 1, 64, 16, 1, P, None) == LAUNCH      # somebody else's failure is on record first
    assert lib.td_last_hip_error().decode().startswith("td_bias_act_fwd: ")
    for name in LAUNCHES:
        code = group_call(lib, [GOOD, dict(K=128, dw_dtype=0)]) if name == "td_conv1x1_wgrad_group" else call(lib, name)
        text = lib.td_last_hip_error().decode()
        assert code == LAUNCH, (name, code)
        assert text.startswith(name + ": ") and len(text) > len(name) + 2, (name, text)
    # both dtypes of a dispatched entry point, and the backward forms that recompute the mask
    for name, changes in (("td_bn_fwd", dict(dtype=0)), ("td_bn_bwd", dict(y=None)), ("td_conv1x1_wgrad", dict(dw_dtype=0)),
                          ("td_join_bwd", dict(dtype=0)), ("td_bn_bwd_from_partials", dict(stat_rows=200, dtype=0))):
        assert call(lib, name, **changes) == LAUNCH and lib.td_last_hip_error().decode().startswith(name + ": "), name


def test_check_quotes_the_hip_text_for_launch_failures_only(lib):
    assert call(lib, "td_bn_fwd_partials") == LAUNCH
    hip = lib.td_last_hip_error().decode()
    assert hip.startswith("td_bn_fwd_partials: ")
    with pytest.raises(native.NativeLibraryError) as launch:
        native.check(LAUNCH, "td_bn_fwd_partials")
    assert "[" + hip + "]" in str(launch.value)
    for code in (BAD, UNS, -4):
        with pytest.raises(native.NativeLibraryError) as other:
            native.check(call(lib, "td_join_fwd", a=None) if code == BAD else code, "td_join_fwd")
        assert hip not in str(other.value) and "[" not in str(other.value) and "(%d)" % code in str(other.value)
