"""csrc/td_align.hip on the device (through tripled_amd.cloud_align) against the numpy statements, which tests/test_cloud_align_cpu.py
pins to a per-point loop and to a per-row loop over the two-stage tree.  Every comparison is exact: np.array_equal on the bits of the
17 sums and of the transformed points, on the counters, and on a whole Alignment (scale, R, t, history, iterations, converged) between
the device path and the host path, whose closed-form solve runs on the host for both and is fed the same bits.  The one place where
bits are not compared is a transformed row that is not finite: 0 inf makes a NaN whose sign the hardware chooses, so those rows are
compared as NaN / inf patterns (np.array_equal(..., equal_nan=True)).

Shapes: the smallest at which the kernels can go wrong.  Points: fewer than a wave, a wave, one more, more than a workgroup, several
workgroups.  Rows of the moments: the same, a full workgroup and one row either side of it (255, 256, 257: one and two partials), and
65 537 rows = 257 partials, the smallest N at which a stage-2 thread adds two partials.  The reference of the moments sits between
guard rows of NaN: a read outside it would poison the sums.  An index beyond 2^31 (52 GB of float64 rows) is not run: all offsets are
64-bit by construction, and an index of 2^40 is among the poisons that must read nothing."""
import ctypes

import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import cloud_align, native
from tests import cloud_align_util as U

pytestmark = pytest.mark.gpu

_HOST = {}


def _dev():
    return torch.device("cuda", 0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _h(t):
    return t.cpu().numpy()


# ---- 1. the transform ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1000])
def test_transform_is_the_numpy_statement(N):
    src = U.points_with_poison(N)
    c, R, t = U.planted("large")
    want = cloud_align.transform_numpy(src, c, R, t)
    finite = np.isfinite(src).all(1)
    buf = torch.zeros(3 * N + 3, dtype=torch.float64, device=_dev())
    for offset in (0, 1):                                              # a 16-byte aligned base pointer, and one that is only 8-byte aligned
        view = buf[offset:offset + 3 * N].view(N, 3)
        view.copy_(_d(src))
        assert view.data_ptr() % 16 == 8 * offset and view.is_contiguous()
        got = cloud_align.transform_hip(view, c, R, t)
        assert got.dtype == torch.float64 and got.shape == (N, 3) and got.data_ptr() != view.data_ptr()
        got = _h(got)
        assert U.same_bits(got[finite], want[finite]) and np.array_equal(got, want, equal_nan=True)
        assert not np.isfinite(got[~finite]).all(1).any() and np.array_equal(_h(view), src, equal_nan=True)
    into = cloud_align.transform_hip(view, c, R, t, out=view)          # in place
    assert into.data_ptr() == view.data_ptr() and U.same_bits(_h(view)[finite], want[finite]) and float(buf[-1]) == 0.0
    if N == 1000:
        assert (~finite).sum() == 3
    none = cloud_align.transform_hip(torch.zeros(0, 3, dtype=torch.float64, device=_dev()), c, R, t)
    assert none.shape == (0, 3)


# ---- 2. the moments ------------------------------------------------------------------------------------------------------------------

def _moments_on_device(cur, ref, index, d2, trim2, origin, guard=7):
    fenced = torch.full((len(ref) + 2 * guard, 3), float("nan"), dtype=torch.float64, device=_dev())
    fenced[guard:guard + len(ref)] = _d(ref)
    inside = fenced[guard:guard + len(ref)]
    out = cloud_align.moments_hip(_d(cur), inside, _d(index), _d(d2), trim2, origin)
    assert out.dtype == torch.float64 and out.shape == (19,)
    host = _h(fenced)
    assert np.isnan(host[:guard]).all() and np.isnan(host[guard + len(ref):]).all() and np.array_equal(host[guard:guard + len(ref)], ref)
    return cloud_align.moments_to_host(out)


@pytest.mark.parametrize("kind", ["mixed", "matched", "unmatched"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000, 65537])
def test_moments_are_the_numpy_statement(N, kind):
    args = U.correspondences(N, kind=kind)
    want_m, want_matched, want_bad = cloud_align.moments_numpy(*args)
    m, matched, bad = _moments_on_device(*args)
    assert U.same_bits(m, want_m) and (matched, bad) == (want_matched, want_bad)
    again = _moments_on_device(*args)                                  # twice in a row: identical bits
    assert U.same_bits(again[0], m) and again[1:] == (matched, bad)
    if kind == "matched":
        assert matched == N and bad == 0 and np.isfinite(m).all()
    elif kind == "unmatched":
        assert matched == 0 and bad == 0 and U.same_bits(m, np.zeros(17))
    elif N >= 63:
        cur, ref, index, d2, trim2, _ = args
        assert 0 < matched < N and bad == 3 and np.isfinite(m).all()
        assert (index == len(ref)).any() and (index == 2 ** 40).any() and (index == -2).any() and (index == len(ref) - 1).any()
        at = np.nonzero(d2 == trim2)[0]
        assert len(at) == 1 and index[at[0]] == 0                       # a d2 exactly at trim2 is matched: without it the sum differs
        without = d2.copy()
        without[at[0]] = np.inf
        assert not U.same_bits(cloud_align.moments_numpy(cur, ref, index, without, trim2, args[5])[0], want_m)


def test_no_rows_zero_the_output_and_no_reference_matches_nothing():
    cur, ref, index, d2, trim2, origin = U.correspondences(65)
    out = torch.full((19,), 7.5, dtype=torch.float64, device=_dev())
    none = torch.zeros(0, 3, dtype=torch.float64, device=_dev())
    got = cloud_align.moments_hip(none, _d(ref), _d(index[:0]), _d(d2[:0]), trim2, origin, out=out)
    assert got.data_ptr() == out.data_ptr() and not _h(out).view(np.uint64).any()
    m, matched, bad = cloud_align.moments_to_host(cloud_align.moments_hip(_d(cur), none, _d(index), _d(d2), trim2, origin))
    want = cloud_align.moments_numpy(cur, ref[:0], index, d2, trim2, origin)
    assert U.same_bits(m, want[0]) and (matched, bad) == want[1:] == (0, int(np.count_nonzero(index != -1)))
    lib = native.load()
    out.fill_(7.5)                                                     # the entry point itself, with nothing but an origin and out
    assert lib.td_icp_moments(None, 0, None, 0, None, None, trim2, (ctypes.c_double * 3)(), None, 0, out.data_ptr(), native.stream()) == 0
    assert not _h(out).view(np.uint64).any()


# ---- 3. the loop -----------------------------------------------------------------------------------------------------------------------

def _host(which, **kw):
    key = (which,) + tuple(sorted(kw.items()))
    if key not in _HOST:
        pred, ref, _ = U.street_pair(which)
        _HOST[key] = cloud_align.align_numpy(pred, ref, U.STREET_TAU, **kw)
    return _HOST[key]


def _identical(a, b):
    return (a.scale == b.scale and np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t) and a.history == b.history and
            a.iterations == b.iterations and a.converged == b.converged)


@pytest.mark.parametrize("which", ["small", "large"])
def test_aligner_on_the_device_is_the_host_path_exactly(which):
    pred, ref, planted = U.street_pair(which)
    want = _host(which)
    aligner = cloud_align.CloudAligner(_dev(), U.STREET_TAU)
    first, second = aligner.align(pred, ref), aligner.align(_d(pred), _d(ref))
    assert isinstance(first.scale, float) and isinstance(first.R, np.ndarray) and first.R.shape == (3, 3) and first.t.shape == (3,)
    assert _identical(first, want) and _identical(second, first)
    assert want.converged and want.history[-1][0] == len(pred) and abs(want.scale - planted[0]) <= 1e-9 * planted[0]


def test_stride_passes_running_out_rigid_mode_and_an_initial_guess():
    pred, ref, planted = U.street_pair("large")
    tau = U.STREET_TAU
    assert _identical(cloud_align.CloudAligner(_dev(), tau, stride=3).align(pred, ref), _host("large", stride=3))
    short = cloud_align.CloudAligner(_dev(), tau, iters=10).align(pred, ref)
    assert _identical(short, _host("large", iters=10)) and not short.converged and short.iterations == 10
    rigid = cloud_align.CloudAligner(_dev(), tau, mode="rigid", trim=tau / 2).align(pred, ref)
    assert _identical(rigid, _host("large", mode="rigid", trim=tau / 2)) and rigid.scale == 1.0
    at_once = cloud_align.CloudAligner(_dev(), tau).align(pred, ref, init=planted)
    assert at_once.converged and at_once.iterations == 1
    far = cloud_align.CloudAligner(_dev(), tau).align(pred[:50] + 100.0, ref)      # nothing matched: the solve is degenerate
    assert not far.converged and far.history == ((0, 0.0),) and far.scale == 1.0 and np.array_equal(far.R, np.eye(3))


def test_cpu_tensors_raise():
    cur, ref, index, d2, trim2, origin = U.correspondences(8)
    c, R, t = U.planted("small")
    with pytest.raises(native.NativeLibraryError):
        cloud_align.transform_hip(torch.from_numpy(cur), c, R, t)
    with pytest.raises(native.NativeLibraryError):
        cloud_align.transform_hip(_d(cur), c, R, t, out=torch.zeros(8, 3, dtype=torch.float64))
    for host in range(4):
        tensors = [_d(a) if k != host else torch.from_numpy(a) for k, a in enumerate((cur, ref, index, d2))]
        with pytest.raises(native.NativeLibraryError):
            cloud_align.moments_hip(*tensors, trim2, origin)
    with pytest.raises(ValueError):
        cloud_align.transform_hip(_d(cur).float(), c, R, t)
    with pytest.raises(ValueError):
        cloud_align.moments_hip(_d(cur), _d(ref), _d(index).int(), _d(d2), trim2, origin)
    with pytest.raises(native.NativeLibraryError):
        cloud_align.transform_hip(_d(cur), float("nan"), R, t)          # refused by the entry point, before any launch
