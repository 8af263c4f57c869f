"""csrc/td_cloud.hip on the device (through tripled_amd.cloud) against the numpy statements, which tests/test_cloud_cpu.py pins to a
brute-force per-point fusion.  Every comparison is exact (np.array_equal on keys, payloads, sums, the bits of xyz, rgb and count):
every quantity is an integer or a fixed sequence of individually rounded float64 operations.

Shapes: the smallest at which each kernel can go wrong.  Keys: rows shorter than a vector (13), longer than a wave (70: vector width
2), longer than a workgroup's run (257: width 1), a row that takes the widest vector over several workgroups (264: width 4), and the
same behind an unaligned base pointer (the scalar path).  Segmented sum: a wave walks 64 elements at a time through a stretch of
512, a workgroup holds four stretches; the run layouts put run starts and ends on each of those boundaries.  An index beyond 2^31
(8.6 GB of depth alone, 40 GB with keys and payloads) is not run: all offsets are 64-bit by construction."""
import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import cloud, native
from tests import cloud_util as U
from tests import odom_util
from tests.infer_util import build_model, randomize_batchnorm

pytestmark = pytest.mark.gpu

INVALID = cloud.INVALID_KEY


def _dev():
    return torch.device("cuda", 0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _h(t):
    return t.cpu().numpy()


# ---- 1. keys -----------------------------------------------------------------------------------------------------------------------

def _check_keys(depth, color, poses, inv_K, params, depth_d=None, color_d=None):
    want_key, want_payload, want_counts = cloud.keys_numpy(depth, color, poses, inv_K, inv_voxel=1.0 / U.VOXEL, **params)
    stats = torch.zeros(6, dtype=torch.int64, device=_dev())
    key, payload = cloud.keys_hip(_d(depth) if depth_d is None else depth_d, _d(color) if color_d is None else color_d, _d(poses), inv_K,
                                  inv_voxel=1.0 / U.VOXEL, stats=stats, **params)
    assert key.dtype == torch.int64 and payload.dtype == torch.int64
    assert np.array_equal(_h(key), want_key)
    assert np.array_equal(_h(payload).view(np.uint64), want_payload)
    assert np.array_equal(_h(stats), want_counts)
    return want_counts


@pytest.mark.parametrize("edge", [0.0, 0.15])
@pytest.mark.parametrize("border", [0, 2])
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("H,W", [(7, 13), (9, 70), (5, 257), (6, 264)])
def test_keys_are_the_numpy_statement(H, W, stride, border, edge):
    depth, color, poses, inv_K = U.scene(H * W + stride, 3, H, W)
    counts = _check_keys(depth, color, poses, inv_K, dict(U.PARAMS, stride=stride, border=border, edge=edge))
    # the inputs do exercise the causes: bad depths, a step edge, points beyond the key range (the far frame), negative coordinates
    assert (counts[1] > 0) == (stride > 1) and (stride > 1 or (counts[2] > 0) == (border > 0))
    if stride == 1 and border == 0:
        assert counts[0] > 0 and counts[3] > 0 and counts[5] > 0 and (counts[4] > 0) == (edge > 0)
        key = cloud.keys_numpy(depth, color, poses, inv_K, inv_voxel=1.0 / U.VOXEL, **dict(U.PARAMS, edge=edge))[0]
        assert min(int(c.min()) for c in cloud.unpack_key(key[key != INVALID])) < 0


def test_keys_behind_an_unaligned_base_pointer():
    """A slice one element into a buffer: no vector width fits the base pointers, so the scalar path runs on a row length (264) that
    otherwise takes the widest one.  Scales other than 1 ride along."""
    B, H, W = 3, 6, 264
    depth, color, poses, inv_K = U.scene(11, B, H, W)
    dbuf = torch.zeros(B * H * W + 1, dtype=torch.float32, device=_dev())
    cbuf = torch.zeros(B * 3 * H * W + 1, dtype=torch.uint8, device=_dev())
    dbuf[1:].copy_(_d(depth).reshape(-1))
    cbuf[1:].copy_(_d(color).reshape(-1))
    depth_d, color_d = dbuf[1:].view(B, H, W), cbuf[1:].view(B, 3, H, W)
    assert depth_d.data_ptr() % 8 == 4 and color_d.data_ptr() % 2 == 1 and depth_d.is_contiguous()
    _check_keys(depth, color, poses, inv_K, dict(U.PARAMS, edge=0.2, border=1, depth_scale=1.3, pose_scale=0.7), depth_d, color_d)


def test_keys_of_no_frames():
    key, payload = cloud.keys_hip(torch.zeros(0, 4, 6, device=_dev()), torch.zeros(0, 3, 4, 6, dtype=torch.uint8, device=_dev()),
                                  torch.zeros(0, 3, 4, dtype=torch.float64, device=_dev()), np.eye(3))
    assert key.shape == (0,) and payload.shape == (0,)


# ---- 2. heads and the segmented sum ----------------------------------------------------------------------------------------------

def _keys_of_runs(runs, n=None, tail_invalid=0):
    """Ascending keys with the given run lengths (cut to n elements), negative voxel coordinates included, then invalid keys."""
    cells = np.arange(len(runs)) - len(runs) // 2
    key = np.repeat(cloud.pack_key(cells, -cells, 3 * cells), np.asarray(runs, np.int64))
    key = key[:n] if n is not None else key
    return np.concatenate([key, np.full(tail_invalid, INVALID, np.int64)])


def _fill(pattern, n):
    runs = []
    while sum(runs) < n:
        runs.extend(pattern)
    return runs


def _sources(n, seed, big=False):
    g = np.random.default_rng(seed)
    q, c = g.integers(0, 1024, (n, 3), dtype=np.uint64), g.integers(0, 256, (n, 3), dtype=np.uint64)
    payload = q[:, 0] | (q[:, 1] << np.uint64(10)) | (q[:, 2] << np.uint64(20)) | (c[:, 0] << np.uint64(30)) | \
        (c[:, 1] << np.uint64(38)) | (c[:, 2] << np.uint64(46))
    rows = cloud.unpack_payload(payload) * (g.integers(1, 9, (n, 1)) if not big else 2 ** 31)      # big: counts of 2^31 per row
    return payload, rows


def _check_table(sorted_key, seed, big=False):
    """Both entry points on a shuffled copy of the sorted layout (the sort restores it; the permutation is the gather)."""
    n = len(sorted_key)
    g = np.random.default_rng(seed)
    order = g.permutation(n)
    key = sorted_key[order]
    payload, rows = _sources(n, seed + 1, big)
    flags = _h(cloud.heads_hip(_d(sorted_key)))
    want_flags = (sorted_key != INVALID) & (np.concatenate([[True], sorted_key[1:] != sorted_key[:-1]]))
    assert flags.dtype == np.int32 and np.array_equal(flags, want_flags.astype(np.int32))
    for src in ([rows] if big else [payload, rows]):
        want_keys, want_sums = cloud.voxel_table_numpy(key, src)
        got_keys, got_sums = cloud.table_hip(_d(key), _d(src.view(np.int64) if src.ndim == 1 else src))
        assert got_sums.shape == (len(want_keys), 7) and got_sums.dtype == torch.int64
        assert np.array_equal(_h(got_keys), want_keys) and np.array_equal(_h(got_sums), want_sums)
    return want_sums


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4097])
@pytest.mark.parametrize("layout", ["one", "distinct", "mix"])
def test_segmented_sum(layout, n):
    runs = {"one": [n], "distinct": [1] * n, "mix": _fill([1, 64, 65, 1500, 1, 1, 63], n)}[layout]
    sums = _check_table(_keys_of_runs(runs, n), n)
    if layout == "one":
        assert sums.shape == (1, 7)          # n = 4097: one run across every 64-element step, wave stretch and workgroup


@pytest.mark.parametrize("runs", [
    [511, 700, 1, 300],                  # a run that starts on the last element of a wave's stretch and crosses the next one whole
    [512, 512, 1, 2047, 1],              # runs that start and end exactly on stretch and workgroup boundaries
    [64, 64, 64, 5, 59, 1, 63, 129],     # runs that end on lane 63: the carried run is flushed at the next step
    [63, 1, 64, 2, 62, 448, 1, 511, 1],  # single elements on lane 63, on the last element of a stretch and on its first
    [1023, 1, 1024, 1, 3000],            # a run over two stretches ending one short, a singleton, a run over two whole stretches
])
def test_segmented_sum_on_the_boundaries(runs):
    _check_table(_keys_of_runs(runs), len(runs))


@pytest.mark.parametrize("n,tail", [(0, 1), (0, 700), (5, 1), (512, 3), (511, 600), (1000, 4097)])
def test_segmented_sum_with_invalid_keys_at_the_tail(n, tail):
    sums = _check_table(_keys_of_runs(_fill([3, 1, 70], n), n, tail), n + tail)
    if n == 0:
        assert sums.shape == (0, 7)          # an all-invalid input: V = 0, nothing is launched


def test_segmented_sum_beyond_32_bits():
    sums = _check_table(_keys_of_runs([3, 1, 600, 2]), 5, big=True)
    assert sums[2, 0] == 600 * 2 ** 31 and sums.max() > 2 ** 40


def test_empty_table():
    keys, sums = cloud.table_hip(torch.zeros(0, dtype=torch.int64, device=_dev()), torch.zeros(0, dtype=torch.int64, device=_dev()))
    assert keys.shape == (0,) and sums.shape == (0, 7)


# ---- 3. merge ----------------------------------------------------------------------------------------------------------------------

def _voxel_list(cells, seed):
    cells = np.asarray(sorted(cells))
    g = np.random.default_rng(seed)
    return cloud.pack_key(cells, 2 * cells, -cells), g.integers(1, 2 ** 33, (len(cells), 7))


@pytest.mark.parametrize("a,b", [
    (range(-300, 0), range(0, 700)),                    # disjoint
    (range(-400, 400), range(-400, 400)),               # identical
    (range(-600, 600, 2), range(-599, 600, 3)),         # interleaved, some shared
    (range(0), range(-5, 900)),                         # an empty list merged into a non-empty one
    (range(-5, 900), range(0)),
])
def test_merge(a, b):
    (ka, sa), (kb, sb) = _voxel_list(a, 1), _voxel_list(b, 2)
    want_keys, want_sums = cloud.voxel_table_numpy(np.concatenate([ka, kb]), np.concatenate([sa, sb]))
    keys, sums = cloud.merge_hip(_d(ka), _d(sa.reshape(-1, 7)), _d(kb), _d(sb.reshape(-1, 7)))
    assert np.array_equal(_h(keys), want_keys) and np.array_equal(_h(sums), want_sums)


# ---- 4. finish ---------------------------------------------------------------------------------------------------------------------

def test_finish():
    g = np.random.default_rng(3)
    cells = g.integers(-cloud.HALF, cloud.HALF, (500, 3))
    n = g.integers(1, 5000, 500)
    sums = np.concatenate([n[:, None], (g.random((500, 3)) * 1023 * n[:, None]).astype(np.int64),
                           (g.random((500, 3)) * 255 * n[:, None]).astype(np.int64)], 1)
    keys = cloud.pack_key(cells[:, 0], cells[:, 1], cells[:, 2])
    # colour means on exact halves, a count that saturates, counts around min_count
    special = np.array([[2, 0, 1023, 1, 1, 3, 510], [2 ** 31, 0, 0, 0, 2 ** 30, 2 ** 31, 255 * 2 ** 31], [4, 6, 6, 6, 5, 6, 7],
                        [2 ** 31 - 1, 5, 5, 5, 2 ** 30, 2 ** 30 - 1, 2 ** 30 + 1], [3, 3, 3, 3, 3, 3, 3]], np.int64)
    sums[:5], n[:5] = special, special[:, 0]
    for min_count in (1, 3, 2 ** 31):
        want = cloud.finish_numpy(keys, sums, 0.37, min_count)
        got = cloud.finish_hip(_d(keys), _d(sums), 0.37, min_count)
        assert np.array_equal(_h(got[0]).view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(_h(got[1]), want[1]) and np.array_equal(_h(got[2]), want[2])
        assert np.array_equal(_h(got[3]).astype(bool), want[3])
    assert want[1][:3].tolist() == [[1, 2, 255], [1, 1, 255], [1, 2, 2]] and want[2][1] == 2 ** 31 - 1 and want[3][:5].tolist() == [
        False, True, False, False, False]
    empty = cloud.finish_hip(_d(keys[:0]), _d(sums[:0]), 0.37)
    assert [tuple(t.shape) for t in empty] == [(0, 3), (0, 3), (0,), (0,)]


# ---- 5. the fusion: reproducible, independent of the batches ----------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W,over", [
    (4, 9, 70, dict(edge=0.2, border=1)),
    (4, 40, 264, dict(stride=2, min_count=2)),
    (3, 192, 640, dict(edge=0.1, voxel=0.25)),   # a training-size frame: 369 k points, runs of 1 to hundreds, hundreds of workgroups
])
def test_fusion_is_reproducible_and_batch_invariant(B, H, W, over):
    depth, color, poses, inv_K = U.scene(B + H, B, H, W, far=False)
    params = dict(U.PARAMS, **over)
    voxel = params.pop("voxel", U.VOXEL)
    want = cloud.fuse_numpy(depth, color, poses, inv_K, voxel, **params)
    assert int(want.count.max()) > 1 and want.stats["valid"] > 0
    dev = (_d(depth), _d(color), _d(poses))
    whole = cloud.fuse_hip(*dev, inv_K, voxel, **params)
    again = cloud.fuse_hip(*dev, inv_K, voxel, **params)
    halves = cloud.fuse_hip(*dev, inv_K, voxel, batch_size=2, **params)
    ones = cloud.fuse_hip(*dev, inv_K, voxel, batch_size=1, **params)
    assert whole.xyz.is_cuda and whole.xyz.dtype == torch.float32 and whole.rgb.dtype == torch.uint8 and whole.count.dtype == torch.int32
    for other in (again, halves, ones, want):
        U.assert_clouds_equal(whole, other)
    assert bool((whole.keys[1:] > whole.keys[:-1]).all())


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------------

FUSER = dict(voxel=0.02, batch_size=4, stride=1, border=2, min_depth=0.1, max_range=50.0, edge=0.5)


def test_scene_fuser_end_to_end(tmp_path):
    """The device cloud against fuse_numpy on the fuser's OWN depth maps and poses, read back: exact.  (The host path's network output
    differs from the device's by MIOpen rounding, so the two paths' clouds are not compared.)"""
    from mono.datasets import KITTIOdomDataset, odom_sequence_files
    gt = odom_util.make_sequence_tree(str(tmp_path), 9, 6, h=64, w=96)
    ds = KITTIOdomDataset(str(tmp_path), odom_sequence_files(9, 6), 64, 96, [0, 1], is_train=False, img_ext=".png")
    model = randomize_batchnorm(build_model("cfg_kitti_fm", 64, 96, seed=3))
    fuser = cloud.SceneFuser(model, 64, 96, _dev(), **FUSER)
    debug = {}
    got = fuser.fuse(ds, debug=debug)
    assert not next(model.parameters()).is_cuda
    depth, poses = debug["depth"], debug["poses"]
    assert depth.is_cuda and depth.shape == (6, 64, 96) and depth.dtype == torch.float32
    assert poses.is_cuda and poses.shape == (6, 3, 4) and poses.dtype == torch.float64
    frames = cloud.odometry.dataset_frames_u8(ds).numpy()
    inv_K = cloud.dataset_inv_K(ds)
    params = {k: v for k, v in FUSER.items() if k not in ("voxel", "batch_size")}
    want = cloud.fuse_numpy(_h(depth), frames, _h(poses), inv_K, FUSER["voxel"], **params)
    assert got.xyz.is_cuda and got.stats["points"] == 6 * 64 * 96 and got.stats["valid"] > 0 and len(want.keys) > 0
    U.assert_clouds_equal(got, want)
    # ground-truth poses, a window of frames, two points per voxel at least
    fuser = cloud.SceneFuser(model, 64, 96, _dev(), min_count=2, depth_scale=1.5, **FUSER)
    sub = fuser.fuse(ds, poses=gt, frames=(1, 6), debug=debug)
    assert np.array_equal(_h(debug["poses"]), gt) and debug["depth"].shape == (5, 64, 96)
    U.assert_clouds_equal(sub, cloud.fuse_numpy(_h(debug["depth"]), frames[1:6], gt[1:6], inv_K, FUSER["voxel"], min_count=2, depth_scale=1.5,
                                                **params))


# ---- 7. the device-only contract ---------------------------------------------------------------------------------------------------

def test_host_tensors_are_refused():
    depth, color, poses, inv_K = U.scene(0, 2, 4, 6)
    key = torch.zeros(4, dtype=torch.int64)
    rows = torch.zeros(4, 7, dtype=torch.int64)
    with pytest.raises(native.NativeLibraryError):
        cloud.keys_hip(_d(depth), torch.from_numpy(color), _d(poses), inv_K)
    with pytest.raises(native.NativeLibraryError):
        cloud.heads_hip(key)
    with pytest.raises(native.NativeLibraryError):
        cloud.reduce_hip(key.to(_dev()), key, None, key.to(_dev()), 1)
    with pytest.raises(native.NativeLibraryError):
        cloud.finish_hip(key.to(_dev()), rows, 0.25)
    with pytest.raises(native.NativeLibraryError):
        cloud.merge_hip(key.to(_dev()), rows.to(_dev()), key, rows)
    with pytest.raises(ValueError):
        cloud.reduce_hip(key.to(_dev()), key.to(_dev()), None, key.to(_dev()), 5)          # more rows than elements
    with pytest.raises(ValueError):
        cloud.keys_hip(_d(depth), _d(color), _d(poses).float(), inv_K)
