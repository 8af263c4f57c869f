"""csrc/td_scan.hip and csrc/td_nn.hip on the device (through tripled_amd.cloud_eval) against the numpy statements, which
tests/test_cloud_eval_cpu.py pins to an all-pairs search and to a per-point loop.  Every comparison is exact (np.array_equal on keys,
payloads, the bits of d2, indices and counters): every quantity is an integer or a fixed sequence of individually rounded float64
operations.  The two means of a Comparison are float64 sums in an order torch chooses: rtol = 1e-12.

Shapes: the smallest at which the kernels can go wrong.  Queries: fewer than a wave, a wave, one more, more than a workgroup, several
workgroups; references of one point (C = 1), of a wave and of 4097 points; a reference that is one cell of 1500 points (the longest
walk) and one with every point in a cell of its own; cells at both ends of the key range, where neighbour cells do not exist; no
reference, no queries; 1 and 16 thresholds, thresholds that equal a distance that occurs.  Scans: lengths 0, 1, 65 and 1000 in one
batch (an empty scan, a scan shorter than a wave, the binary search over several workgroups), behind a 16-byte aligned and an
unaligned base pointer.  An index beyond 2^31 (52 GB of float64 queries alone) is not run: all offsets are 64-bit by construction."""
import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import cloud, cloud_eval, native
from tests import cloud_eval_util as U

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _h(t):
    return t.cpu().numpy()


def _check_nearest(query, ref, tau, thresholds=None):
    """The device's answer is the statement's, and the device's grid is the statement's up to the order inside a cell."""
    want_grid = cloud_eval.grid_numpy(ref, tau)
    want = cloud_eval.nearest_numpy(query, want_grid, tau, thresholds)
    grid = cloud_eval.grid_hip(_d(ref), tau)
    assert grid.stats == want_grid.stats
    assert np.array_equal(_h(grid.cell_key), want_grid.cell_key) and np.array_equal(_h(grid.cell_start), want_grid.cell_start)
    order = _h(grid.order)
    assert np.array_equal(np.sort(order), np.sort(want_grid.order)) and np.array_equal(_h(grid.points), np.asarray(ref, np.float64)[order])
    got = cloud_eval.nearest_hip(_d(query), grid, tau, thresholds)
    assert got.d2.dtype == torch.float64 and got.index.dtype == torch.int64 and got.counts.dtype == torch.int64
    assert np.array_equal(_h(got.d2).view(np.uint64), want.d2.view(np.uint64))
    assert np.array_equal(_h(got.index), want.index)
    assert np.array_equal(_h(got.counts), want.counts)
    return want


# ---- 1. nearest neighbour --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 64, 4097])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1000])
def test_nearest_is_the_numpy_statement(N, M):
    tau = 0.25
    query, ref = U.random_scene(N, M, tau, seed=N + M)
    want = _check_nearest(query, ref, tau)
    if N >= 63 and M >= 64:
        assert 0 < want.counts[3] < N and want.counts[4] == 0          # found and not found both occur


@pytest.mark.parametrize("tau", U.TAUS)
def test_lattice_ties_radius_copies_duplicates_and_unusable_queries(tau):
    """The scene of the CPU test, which the all-pairs search pins there."""
    query, ref = U.nn_scene(tau)
    want = _check_nearest(query, ref, tau)
    assert want.counts[4] == 4 and 0 < want.counts[0] < want.counts[3] < len(query) - 4


def test_one_cell_of_1500_points_and_cells_of_one_point():
    tau = 0.5
    rng = np.random.default_rng(5)
    crowd = rng.uniform(0.05, 0.3, (1500, 3))                          # one cell: floor(x (1 - 2^-20) / 0.5) = 0 on every axis
    query = np.concatenate([rng.uniform(-0.6, 0.9, (257, 3)), crowd[::50]])
    want = _check_nearest(query, crowd, tau)
    grid = cloud_eval.grid_numpy(crowd, tau)
    assert grid.stats["cells"] == 1 and grid.stats["max_cell"] == 1500 and 0 < want.counts[3] < len(query)
    alone = np.stack(np.meshgrid(*[np.arange(-6, 6) * 1.25] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.1      # 1728 cells of one point
    query = alone[::3] + rng.normal(0, 0.3, (576, 3))
    want = _check_nearest(query, alone, tau)
    assert cloud_eval.grid_numpy(alone, tau).stats["max_cell"] == 1 and 0 < want.counts[3] < len(query)


def test_cells_at_both_ends_of_the_key_range():
    """tau = 1: the last cell on an axis starts at 2^20 - 2^-20 and the first one ends at -2^20 - 1 + ...; a neighbour cell beyond
    either does not exist and is skipped, a point or a query beyond either is dropped or invalid.  The all-top corner cell's key is
    the sentinel: reference points in it are dropped, queries in it are valid."""
    tau, edge = 1.0, float(2 ** 20)
    rng = np.random.default_rng(9)

    def around(n):
        base = rng.uniform(-2.0, 2.0, (n, 3))
        side = rng.integers(0, 4, (n, 3))                              # per axis: the top edge, the bottom edge, or the middle
        return base + np.where(side == 0, edge, np.where(side == 1, -edge, 0.0)) + np.where(side == 1, -0.5, 0.0)

    ref = np.concatenate([around(3000), np.full((3, 3), edge + 0.25), [[edge + 0.25, edge + 0.25, edge - 0.5]]])
    query = np.concatenate([around(1000), np.full((2, 3), edge + 0.3), [[edge + 0.3, edge + 0.3, edge - 0.3]]])
    want = _check_nearest(query, ref, tau)
    grid = cloud_eval.grid_numpy(ref, tau)
    ix = np.stack(cloud.unpack_key(grid.cell_key), -1)
    assert ix.max() == cloud.HALF - 1 and ix.min() == -cloud.HALF and grid.stats["dropped"] > 3
    assert 0 < want.counts[4] < 1000 and 0 < want.counts[3]
    assert (want.index[-3:] >= 0).all() and (want.index[-3:] < len(ref) - 4).sum() + (want.index[-3:] == len(ref) - 1).sum() == 3
    # ^ the corner cell holds nothing (its three points were dropped), yet queries in it are served from the cells next to it


def test_no_reference_and_no_queries():
    tau = 0.25
    query, ref = U.random_scene(65, 64, tau)
    want = _check_nearest(query, np.zeros((0, 3)), tau)
    assert np.isinf(want.d2).all() and (want.index == -1).all() and np.array_equal(want.counts, [0, 0, 0, 0, 0])
    unusable = np.full((5, 3), np.nan)                                 # a reference of which nothing is left: M' = 0 with M > 0
    assert np.array_equal(_check_nearest(query, unusable, tau).counts, [0, 0, 0, 0, 0])
    grid = cloud_eval.grid_hip(_d(ref), tau)
    got = cloud_eval.nearest_hip(torch.zeros(0, 3, dtype=torch.float64, device=_dev()), grid, tau)
    assert got.d2.shape == (0,) and got.index.shape == (0,) and not _h(got.counts).any()


@pytest.mark.parametrize("K", [0, 1, 16])
def test_threshold_counts_and_thresholds_that_equal_a_distance(K):
    tau = 0.25
    h = U.lattice_step(tau)
    corners, _ = U.lattice(tau)
    mids = corners[:60] + np.array([h / 2, 0.0, 0.0])                 # h / 2 from two corners (or from one): d2 = h h / 4 exactly
    rng = np.random.default_rng(K)
    query = np.concatenate([mids, corners[:20], corners[:100] + rng.normal(0, 0.5 * h, (100, 3))])
    thresholds = {0: (), 1: (h / 2,), 16: tuple(np.sort(np.concatenate([[0.0, h / 2, tau], rng.uniform(0, tau, 13)])))}[K]
    want = _check_nearest(query, corners, tau, thresholds)
    assert want.counts.shape == (K + 2,)
    if K:
        assert np.count_nonzero(want.d2 == (h / 2) * (h / 2)) >= 60     # the threshold's square occurs as a d2 ...
        k = thresholds.index(h / 2)
        assert want.counts[k] >= 80 and want.counts[k] == np.count_nonzero(want.d2 <= (h / 2) * (h / 2))      # ... and is counted
    # a counter tensor of the caller's is incremented, not overwritten
    counts = torch.full((K + 2,), 7, dtype=torch.int64, device=_dev())
    cloud_eval.nearest_hip(_d(query), cloud_eval.grid_hip(_d(corners), tau), tau, thresholds, counts=counts)
    assert np.array_equal(_h(counts), want.counts + 7)


# ---- 2. scans --------------------------------------------------------------------------------------------------------------------

def _check_scan_keys(points, offsets, poses, camera, points_d=None):
    want_key, want_payload, want_counts = cloud_eval.scan_keys_numpy(points, offsets, U.TR, poses, **camera, **U.SCAN_PARAMS)
    stats = torch.zeros(5, dtype=torch.int64, device=_dev())
    key, payload = cloud_eval.scan_keys_hip(_d(points) if points_d is None else points_d, _d(offsets), U.TR, _d(poses), stats=stats,
                                            **camera, **U.SCAN_PARAMS)
    assert key.dtype == torch.int64 and payload.dtype == torch.int64
    assert np.array_equal(_h(key), want_key)
    assert np.array_equal(_h(payload).view(np.uint64), want_payload)
    assert np.array_equal(_h(stats), want_counts)
    return want_counts


@pytest.mark.parametrize("view", [False, True])
def test_scan_keys_are_the_numpy_statement(view):
    points, offsets, poses = U.scan_batch((0, 1, 65, 1000))
    camera = dict(K=U.scan_K(), height=U.SCAN_H, width=U.SCAN_W) if view else {}
    counts = _check_scan_keys(points, offsets, poses, camera)
    assert counts[0] > 0 and counts[1] == 6 and counts[2] > 0 and (counts[3] > 0) == view and counts[4] > 0
    # the same behind a base pointer that is 4-byte but not 16-byte aligned: the scalar loads
    buf = torch.zeros(points.size + 1, dtype=torch.float32, device=_dev())
    buf[1:].copy_(_d(points).reshape(-1))
    shifted = buf[1:].view(-1, 4)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    _check_scan_keys(points, offsets, poses, camera, shifted)


def test_scan_keys_of_points_nobody_owns_and_of_no_points():
    points, offsets, poses = U.scan_batch((5, 40))
    short = offsets.copy()
    short[0], short[-1] = 2, 40                                         # points 0, 1 and 40 ... 44 belong to no scan
    key, _ = cloud_eval.scan_keys_hip(_d(points), _d(short), U.TR, _d(poses), **U.SCAN_PARAMS)
    want = cloud_eval.scan_keys_numpy(points, short, U.TR, poses, **U.SCAN_PARAMS)
    assert np.array_equal(_h(key), want[0]) and (want[0][[0, 1, 40, 44]] == cloud.INVALID_KEY).all() and want[2][1] >= 7
    none = torch.zeros(0, 4, dtype=torch.float32, device=_dev())
    key, payload = cloud_eval.scan_keys_hip(none, _d(np.zeros(2, np.int64)), U.TR, _d(poses[:1]), **U.SCAN_PARAMS)
    assert key.shape == (0,) and payload.shape == (0,)


def test_scan_fuser_does_not_depend_on_the_batch_size():
    points, offsets, poses = U.scan_batch((0, 1, 65, 1000))
    scans = [points[offsets[s]:offsets[s + 1]] for s in range(4)]
    args = dict(K=U.scan_K(), height=U.SCAN_H, width=U.SCAN_W, min_depth=1.0, max_range=45.0)
    want = cloud_eval.ScanFuser("cpu", U.SCAN_VOXEL, U.TR, **args).fuse(scans, poses)
    assert want.stats["valid"] > 0 and want.stats["voxels"] == len(want.keys) > 0
    for batch_size in (4, 2, 1):
        got = cloud_eval.ScanFuser(_dev(), U.SCAN_VOXEL, U.TR, batch_size=batch_size, **args).fuse(scans, poses)
        assert got.xyz.is_cuda and got.stats == want.stats
        assert np.array_equal(_h(got.keys), want.keys) and np.array_equal(_h(got.xyz).view(np.uint32), want.xyz.view(np.uint32))
        assert np.array_equal(_h(got.rgb), want.rgb) and np.array_equal(_h(got.count), want.count)


# ---- 3. scores -------------------------------------------------------------------------------------------------------------------

def test_comparer_equals_numpy_and_itself():
    tau = 0.25
    rng = np.random.default_rng(3)
    ref = rng.uniform(-2, 2, (5000, 3)).astype(np.float32)
    pred = np.concatenate([ref[:3000] * np.float32(0.5) + rng.normal(0, 0.03, (3000, 3)).astype(np.float32),
                           rng.uniform(-1.5, 1.5, (1000, 3)).astype(np.float32), [[np.nan, 0, 0]]]).astype(np.float32)
    want = cloud_eval.compare_numpy(pred, ref, tau, pred_scale=2.0)
    comparer = cloud_eval.CloudComparer(_dev(), tau)
    first, second = comparer.compare(pred, ref, pred_scale=2.0), comparer.compare(_d(pred), _d(ref), pred_scale=2.0)
    for got in (first, second):
        assert got.thresholds == want.thresholds and got.precision == want.precision and got.recall == want.recall
        assert got.fscore == want.fscore and got.stats == want.stats
        for a, b in ((got.pred, want.pred), (got.ref, want.ref)):
            assert np.array_equal(a.counts, b.counts) and np.array_equal(_h(a.index), b.index)
            assert np.array_equal(_h(a.d2).view(np.uint64), b.d2.view(np.uint64))
        assert np.isclose(got.accuracy, want.accuracy, rtol=1e-12, atol=0) and np.isclose(got.completeness, want.completeness, rtol=1e-12, atol=0)
    assert first.accuracy == second.accuracy and first.completeness == second.completeness
    assert 0 < want.precision[0] < want.precision[2] < 1 and 0 < want.recall[2] < 1 and want.pred.counts[4] == 1


def test_wall_on_the_device():
    scans, poses = U.wall_scans()
    ref = cloud_eval.ScanFuser(_dev(), U.WALL_VOXEL, U.TR, min_depth=1.0, max_range=20.0).fuse(scans, poses)
    pred = U.wall_prediction()
    comparer = cloud_eval.CloudComparer(_dev(), U.WALL_TAU)
    same = comparer.compare(pred, ref.xyz)
    assert same.precision[-1] == 1.0 and same.recall[-1] == 1.0 and same.fscore[-1] == 1.0
    apart = comparer.compare(pred + np.array([0, 0, 2 * U.WALL_TAU], np.float32), ref.xyz)
    assert apart.precision[-1] == 0.0 and apart.recall[-1] == 0.0 and apart.fscore[-1] == 0.0 and apart.accuracy == U.WALL_TAU


def test_cpu_tensors_raise():
    tau = 0.25
    query, ref = U.random_scene(8, 8, tau)
    grid = cloud_eval.grid_hip(_d(ref), tau)
    with pytest.raises(native.NativeLibraryError):
        cloud_eval.grid_hip(torch.from_numpy(ref), tau)
    with pytest.raises(native.NativeLibraryError):
        cloud_eval.nearest_hip(torch.from_numpy(query), grid, tau)
    with pytest.raises(native.NativeLibraryError):
        cloud_eval.nearest_hip(_d(query), grid._replace(order=grid.order.cpu()), tau)
    with pytest.raises(ValueError):
        cloud_eval.nearest_hip(_d(query), grid, 0.5)                    # a grid built for another radius
    with pytest.raises(ValueError):
        cloud_eval.nearest_hip(_d(query).float(), grid, tau)
    points, offsets, poses = U.scan_batch((3, 5))
    with pytest.raises(native.NativeLibraryError):
        cloud_eval.scan_keys_hip(torch.from_numpy(points), _d(offsets), U.TR, _d(poses), **U.SCAN_PARAMS)
    with pytest.raises(native.NativeLibraryError):
        cloud_eval.scan_keys_hip(_d(points), _d(offsets), U.TR, torch.from_numpy(poses), **U.SCAN_PARAMS)
