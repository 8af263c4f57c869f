"""csrc/td_normals.hip and td_icp_plane_moments (csrc/td_align.hip) on the device, through tripled_amd.cloud_normals and
tripled_amd.cloud_align, against the numpy statements that tests/test_cloud_plane_cpu.py pins to per-point and per-row Python loops.
Every comparison is exact: np.array_equal on the bits of the normals, the curvatures and the 37 sums, on the counts and counters, and
on a whole point-to-plane alignment (scale, R, t, history, plane_history with its ranks and dropped directions, pass count, converged)
between the device path and the host path, whose solve runs on the host for both and is fed the same bits.

Shapes: the smallest at which the kernels can go wrong.  Queries: fewer than a wave, a wave, one more, more than a workgroup, several
workgroups, on a cloud with every kind of point planted (not finite, out of key range, isolated, collinear, duplicates, a blob, 300
points in one cell); a lattice whose neighbours lie at exactly the radius and offsets that quantise half way.  Rows of the moments:
the same, a full workgroup and one row either side (255, 256, 257) and 65 537 rows = 257 partials, the smallest N at which a stage-2
thread adds two.  The grid's points lie between guard rows that WOULD count as neighbours if a walk left the cells; the reference and
the normals of the moments between guard rows of NaN, which would poison the sums."""
import ctypes

import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import cloud_align, cloud_eval, cloud_normals, native
from tests import cloud_align_util as U
from tests import cloud_plane_util as P

pytestmark = pytest.mark.gpu

CONFIGS = ((None, 6), (P.NORMAL_TAU / 2, 3))
_HOST = {}


def _dev():
    return torch.device("cuda", 0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _h(t):
    return t.cpu().numpy()


def _same(got, want):
    return (U.same_bits(_h(got.normal), want.normal) and U.same_bits(_h(got.curvature), want.curvature) and
            np.array_equal(_h(got.count), want.count) and np.array_equal(_h(got.stats), want.stats))


def _fenced_grid(x, tau, guard=5):
    """grid_hip's Grid with its points inside a larger buffer whose guard rows repeat the first and the last point."""
    grid = cloud_eval.grid_hip(_d(x), tau)
    M = grid.points.shape[0]
    if M == 0:
        return grid, None
    buf = torch.empty(M + 2 * guard, 3, dtype=torch.float64, device=_dev())
    buf[:guard], buf[guard:guard + M], buf[guard + M:] = grid.points[0], grid.points, grid.points[M - 1]
    return grid._replace(points=buf[guard:guard + M]), buf


# ---- 1. normals ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", P.NORMAL_SIZES)
def test_normals_are_the_numpy_statement(N):
    x = P.poison_cloud(N)
    host_grid = cloud_eval.grid_numpy(x, P.NORMAL_TAU)
    grid, _ = _fenced_grid(x, P.NORMAL_TAU)
    assert np.array_equal(_h(grid.points), host_grid.points) and np.array_equal(_h(grid.cell_start), host_grid.cell_start)
    for radius, least in CONFIGS:
        want = cloud_normals.normals_numpy(x, host_grid, radius, least)
        got = cloud_normals.normals_hip(_d(x), grid, radius, least)
        assert got.normal.dtype == torch.float64 and got.normal.shape == (N, 3) and got.count.dtype == torch.int64 and got.stats.shape == (5,)
        assert _same(got, want), (N, radius)
        again = cloud_normals.normals_hip(_d(x), grid, radius, least, stats=got.stats)      # twice in a row; the counters are incremented
        assert U.same_bits(_h(again.normal), want.normal) and U.same_bits(_h(again.curvature), want.curvature)
        assert again.stats.data_ptr() == got.stats.data_ptr() and np.array_equal(_h(again.stats), 2 * want.stats)
        assert int(want.stats.sum()) == N
    if N == 1000:
        assert _h(got.count).max() == 300 and (want.stats > 0).all()


def test_normals_in_cells_at_both_ends_of_the_key_range():
    """The scene of the CPU test of that name, which the all-pairs loop pins there."""
    query, ref = P.key_range_scene()
    tau = P.KEY_RANGE_TAU
    host_grid = cloud_eval.grid_numpy(ref, tau)
    want = cloud_normals.normals_numpy(query, host_grid, tau, 3, 1.0)
    grid = cloud_eval.grid_hip(_d(ref), tau)
    got = cloud_normals.normals_hip(_d(query), grid, tau, 3, 1.0)
    assert _same(got, want)
    P.check_key_range_grid(grid._replace(cell_key=_h(grid.cell_key)), _h(got.stats))      # the grid that was queried
    P.check_key_range_grid(host_grid, want.stats)


def test_no_queries_the_exact_radius_and_half_way_offsets():
    x = P.poison_cloud(65)
    grid = cloud_eval.grid_hip(_d(x), P.NORMAL_TAU)
    none = cloud_normals.normals_hip(torch.zeros(0, 3, dtype=torch.float64, device=_dev()), grid)
    assert none.normal.shape == (0, 3) and none.count.shape == (0,) and not _h(none.stats).any()
    empty = cloud_eval.grid_hip(torch.zeros(0, 3, dtype=torch.float64, device=_dev()), P.NORMAL_TAU)      # no cloud: every query has few
    alone = cloud_normals.normals_hip(_d(x), empty)
    assert _same(alone, cloud_normals.normals_numpy(x, cloud_eval.grid_numpy(x[:0], P.NORMAL_TAU))) and not _h(alone.count).any()
    sheet = P.lattice_sheet()
    got = cloud_normals.normals_hip(_d(sheet), _fenced_grid(sheet, 0.5)[0], 0.5)
    assert _same(got, cloud_normals.normals_numpy(sheet, cloud_eval.grid_numpy(sheet, 0.5), 0.5))
    assert _h(got.count).max() == 13 and U.same_bits(_h(got.normal), np.tile([0.0, 0.0, 1.0], (81, 1)))
    half, _ = P.half_way_cloud(0.5)
    got = cloud_normals.normals_hip(_d(half), cloud_eval.grid_hip(_d(half), 0.5), 0.5)
    assert _same(got, cloud_normals.normals_numpy(half, cloud_eval.grid_numpy(half, 0.5), 0.5)) and (_h(got.count) == 12).all()


def test_cloud_normals_on_the_device_is_the_host_path():
    x = U.street(0)
    want = cloud_normals.CloudNormals("cpu", U.STREET_TAU).estimate(x)
    got = cloud_normals.CloudNormals(_dev(), U.STREET_TAU).estimate(x)
    assert got.normal.is_cuda and got.stats == want.stats and got.stats["valid"] > 5000 and got.stats["rough"] > 0
    assert U.same_bits(_h(got.normal), want.normal) and U.same_bits(_h(got.curvature), want.curvature) and np.array_equal(_h(got.count), want.count)


# ---- 2. the plane moments ----------------------------------------------------------------------------------------------------------------

def _plane_moments_on_device(cur, ref, normals, index, d2, trim2, origin, guard=7):
    fenced = torch.full((2, len(ref) + 2 * guard, 3), float("nan"), dtype=torch.float64, device=_dev())
    fenced[0, guard:guard + len(ref)], fenced[1, guard:guard + len(ref)] = _d(ref), _d(normals)
    out = cloud_align.plane_moments_hip(_d(cur), fenced[0, guard:guard + len(ref)], fenced[1, guard:guard + len(ref)], _d(index), _d(d2), trim2, origin)
    assert out.dtype == torch.float64 and out.shape == (40,)
    host = _h(fenced)
    assert np.isnan(host[:, :guard]).all() and np.isnan(host[:, guard + len(ref):]).all() and np.array_equal(host[0, guard:guard + len(ref)], ref)
    return cloud_align.plane_moments_to_host(out)


@pytest.mark.parametrize("kind", ["mixed", "matched", "unmatched"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000, 65537])
def test_plane_moments_are_the_numpy_statement(N, kind):
    args = P.plane_correspondences(N, kind=kind)
    want = cloud_align.plane_moments_numpy(*args)
    got = _plane_moments_on_device(*args)
    assert U.same_bits(got[0], want[0]) and got[1:] == want[1:]
    again = _plane_moments_on_device(*args)                            # twice in a row: identical bits
    assert U.same_bits(again[0], got[0]) and again[1:] == got[1:]
    m, matched, bad, flat = got
    if kind == "matched":
        assert (matched, bad, flat) == (N, 0, 0) and np.isfinite(m).all()
    elif kind == "unmatched":
        assert (matched, bad, flat) == (0, 0, 0) and U.same_bits(m, np.zeros(37))
    elif N >= 63:
        index = args[3]
        assert 0 < matched < N and bad == 3 and flat > 0 and np.isfinite(m).all()
        assert (index == len(args[1])).any() and (index == 2 ** 40).any() and (index == -2).any() and (index == len(args[1]) - 1).any()


def test_no_rows_zero_the_output_and_no_reference_matches_nothing():
    cur, ref, normals, index, d2, trim2, origin = P.plane_correspondences(65)
    out = torch.full((40,), 7.5, dtype=torch.float64, device=_dev())
    none = torch.zeros(0, 3, dtype=torch.float64, device=_dev())
    got = cloud_align.plane_moments_hip(none, _d(ref), _d(normals), _d(index[:0]), _d(d2[:0]), trim2, origin, out=out)
    assert got.data_ptr() == out.data_ptr() and not _h(out).view(np.uint64).any()
    got = cloud_align.plane_moments_to_host(cloud_align.plane_moments_hip(_d(cur), none, none, _d(index), _d(d2), trim2, origin))
    want = cloud_align.plane_moments_numpy(cur, ref[:0], normals[:0], index, d2, trim2, origin)
    assert U.same_bits(got[0], want[0]) and got[1:] == want[1:] == (0, int(np.count_nonzero(index != -1)), 0)
    lib = native.load()
    out.fill_(7.5)                                                     # the entry point itself, with nothing but an origin and out
    assert lib.td_icp_plane_moments(None, 0, None, None, 0, None, None, trim2, (ctypes.c_double * 3)(), None, 0, out.data_ptr(), native.stream()) == 0
    assert not _h(out).view(np.uint64).any()


# ---- 3. the loop -----------------------------------------------------------------------------------------------------------------------

_PAIRS = {"same small": lambda: U.street_pair("small"), "other small": lambda: P.other_pair("small"),
          "other large": lambda: P.other_pair("large"), "corridor": lambda: P.corridor_pair("small")}


def _identical(a, b, ha, hb):
    if not (a.scale == b.scale and np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t) and a.history == b.history and
            a.iterations == b.iterations and a.converged == b.converged and len(ha) == len(hb)):
        return False
    for (rms_a, rank_a, drop_a), (rms_b, rank_b, drop_b) in zip(ha, hb):
        if rms_a != rms_b or rank_a != rank_b or (drop_a is None) != (drop_b is None) or (drop_a is not None and not np.array_equal(drop_a, drop_b)):
            return False
    return True


@pytest.mark.parametrize("which", list(_PAIRS))
def test_plane_aligner_on_the_device_is_the_host_path_exactly(which):
    pred, ref, planted = _PAIRS[which]()
    host = cloud_align.CloudAligner("cpu", U.STREET_TAU, criterion="plane")
    want = host.align(pred, ref)
    aligner = cloud_align.CloudAligner(_dev(), U.STREET_TAU, criterion="plane")
    first = aligner.align(pred, ref)
    first_history, first_stats = aligner.plane_history, aligner.normal_stats
    second = aligner.align(_d(pred), _d(ref))
    assert isinstance(first.scale, float) and isinstance(first.R, np.ndarray) and first.R.shape == (3, 3) and first.t.shape == (3,)
    assert _identical(first, want, first_history, host.plane_history) and _identical(second, first, aligner.plane_history, first_history)
    assert first_stats == host.normal_stats == aligner.normal_stats
    assert want.converged and want.iterations <= 10
    ranks = [rank for _, rank, _ in host.plane_history]
    assert ranks == [6 if which == "corridor" else 7] * want.iterations


def test_rigid_mode_stride_trim_and_a_degenerate_pass():
    pred, ref, planted = P.other_pair("small")
    tau = U.STREET_TAU
    for kw in (dict(mode="rigid", trim=tau / 2), dict(stride=3, normal_radius=tau / 2, min_neighbours=4, max_curvature=0.05, rcond=1e-2), dict(iters=2)):
        host, device = cloud_align.CloudAligner("cpu", tau, criterion="plane", **kw), cloud_align.CloudAligner(_dev(), tau, criterion="plane", **kw)
        want, got = host.align(pred, ref), device.align(pred, ref)
        assert _identical(got, want, device.plane_history, host.plane_history), kw
    assert got.iterations == 2 and not got.converged
    far = cloud_align.CloudAligner(_dev(), tau, criterion="plane")
    nothing = far.align(pred[:50] + 100.0, ref)                        # nothing matched: the solve is degenerate
    assert not nothing.converged and nothing.history == ((0, 0.0),) and far.plane_history == ((0.0, 0, None),) and nothing.scale == 1.0


def test_cpu_tensors_raise():
    cur, ref, normals, index, d2, trim2, origin = P.plane_correspondences(8)
    for host in range(5):
        tensors = [_d(a) if k != host else torch.from_numpy(a) for k, a in enumerate((cur, ref, normals, index, d2))]
        with pytest.raises(native.NativeLibraryError):
            cloud_align.plane_moments_hip(*tensors, trim2, origin)
    with pytest.raises(ValueError):
        cloud_align.plane_moments_hip(_d(cur), _d(ref), _d(normals).float(), _d(index), _d(d2), trim2, origin)
    with pytest.raises(ValueError):
        cloud_align.plane_moments_hip(_d(cur), _d(ref), _d(normals)[:-1], _d(index), _d(d2), trim2, origin)
    with pytest.raises(native.NativeLibraryError):
        cloud_align.plane_moments_hip(_d(cur), _d(ref), _d(normals), _d(index), _d(d2), trim2, origin, out=torch.zeros(40, dtype=torch.float64))
    x = P.poison_cloud(65)
    grid = cloud_eval.grid_hip(_d(x), P.NORMAL_TAU)
    with pytest.raises(native.NativeLibraryError):
        cloud_normals.normals_hip(torch.from_numpy(x), grid)
    with pytest.raises(native.NativeLibraryError):
        cloud_normals.normals_hip(_d(x), cloud_eval.grid_numpy(x, P.NORMAL_TAU))      # a host grid
    with pytest.raises(native.NativeLibraryError):
        cloud_normals.normals_hip(_d(x), grid, stats=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError):
        cloud_normals.normals_hip(_d(x).float(), grid)
    for bad in (dict(radius=2 * P.NORMAL_TAU), dict(min_neighbours=2), dict(max_curvature=-1.0)):
        with pytest.raises(ValueError):
            cloud_normals.normals_hip(_d(x), grid, **bad)
