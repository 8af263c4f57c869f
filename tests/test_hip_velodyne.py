"""csrc/td_velo.hip on the device (through tripled_amd.velodyne.depth_maps_hip) against the numpy statement, which
tests/test_velodyne_cpu.py pins to a literal per-point loop, to the reference's recorded maps and to maps written down by hand.  Every
comparison is exact: np.array_equal on the float32 bits of the maps and on the stats.  Every table entry of the kernel is a minimum
of integers and the projection a fixed sequence of individually rounded float64 operations.

Shapes: the smallest at which the kernels can go wrong.  Point counts of 1, 63, 65, 257 and 1000 (not a multiple of a wave, just
past a wave, past a workgroup); 600 points on one pixel (more than a workgroup contends for one table entry); maps of 9 x 14 and
12 x 33 in one batch (padding, a resolve block that covers the end of a plane); an unaligned base pointer (the dword path instead
of 16-byte loads).  An index beyond 2^31 is not run: all offsets are 64-bit by construction."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tests import velo_util
from tests.test_velodyne_cpu import golden_scenes
from tripled_amd import native, velodyne

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda", 0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run_batch(frames, vel_depth=False, points_d=None, workspace=None):
    """frames: [(points, P, H, W)] -> (gt [B,Hmax,Wmax], stats [B,6]) as numpy, from ONE call."""
    offsets = np.zeros(len(frames) + 1, np.int64)
    np.cumsum([len(f[0]) for f in frames], out=offsets[1:])
    if points_d is None:
        points_d = _d(np.concatenate([np.asarray(f[0], np.float32).reshape(-1, 4) for f in frames], 0))
    sizes = np.array([[f[2], f[3]] for f in frames], np.int32)
    gt, stats = velodyne.depth_maps_hip(points_d, _d(offsets), _d(np.stack([np.asarray(f[1], np.float64) for f in frames], 0)), _d(sizes),
                                        vel_depth, workspace)
    assert gt.dtype == torch.float32 and stats.dtype == torch.int64
    assert tuple(gt.shape) == (len(frames), int(sizes[:, 0].max()), int(sizes[:, 1].max())) and tuple(stats.shape) == (len(frames), 6)
    return gt.cpu().numpy(), stats.cpu().numpy()


def check_batch(frames, vel_depth=False, **kw):
    """The device batch against the statement, frame by frame: the bits of float32(map), zero padding, the stats."""
    gt, stats = run_batch(frames, vel_depth, **kw)
    for i, (points, P, H, W) in enumerate(frames):
        want, want_stats = velodyne.depth_map_numpy(points, P, H, W, vel_depth)
        assert np.array_equal(_bits(gt[i, :H, :W]), _bits(want.astype(np.float32))), "frame %d" % i
        assert np.array_equal(gt[i, :H, :W], want.astype(np.float32))
        assert not gt[i, H:].any() and not gt[i, :, W:].any(), "frame %d: padding" % i
        assert np.array_equal(stats[i], want_stats), (i, stats[i], want_stats)
    return gt, stats


def _scene(H, W, n, seed, cam=2, specials=True):
    calib = velo_util.synthetic_calibration(H, W, seed)
    return (velo_util.synthetic_scan(calib, n, seed, specials), velo_util.projection(calib, cam), H, W)


@pytest.mark.parametrize("vel_depth", [False, True])
@pytest.mark.parametrize("cam", [2, 3])
def test_golden_scenes(cam, vel_depth):
    for name, calib, points, maps in golden_scenes():
        H, W = velo_util.size_of(calib)
        gt, stats = check_batch([(points, velo_util.projection(calib, cam), H, W)], vel_depth)
        # and the reference's own map: exact with vel_depth, the statement's allowance otherwise (float32 of both sides)
        ref = maps[(cam, vel_depth)].astype(np.float32)
        assert np.array_equal(gt[0] == 0, ref == 0)
        if vel_depth:
            assert np.array_equal(gt[0], ref)
        else:
            np.testing.assert_allclose(gt[0], ref, rtol=2.0 ** -23, atol=0)      # 1e-12 in float64 is at most one float32 step


@pytest.mark.parametrize("vel_depth", [False, True])
def test_mixed_sizes_in_one_batch(vel_depth):
    gt, stats = check_batch([_scene(9, 14, 400, 1), _scene(12, 33, 3000, 2, cam=3), _scene(9, 14, 257, 3)], vel_depth)
    assert gt.shape == (3, 12, 33) and stats[:, 3].min() > 0


def test_a_middle_frame_without_points():
    empty = (np.zeros((0, 4), np.float32), velo_util.PERMUTE, 5, 7)
    gt, stats = check_batch([_scene(9, 14, 400, 1), empty, _scene(6, 9, 300, 5)])
    assert not gt[1].any() and not stats[1].any() and stats[2, 3] > 0


def test_a_frame_without_valid_points():
    none_valid = velo_util.hand_cases()["none_valid"]
    gt, stats = check_batch([_scene(9, 14, 400, 1), none_valid[:4], _scene(6, 9, 300, 5)])
    assert not gt[1].any() and stats[1].tolist() == [3, 2, 1, 0, 0, 0]
    gt, stats = check_batch([(np.zeros((0, 4), np.float32), velo_util.PERMUTE, 5, 7)])      # no point in the whole batch
    assert not gt.any() and not stats.any()


@pytest.mark.parametrize("n", [1, 63, 65, 257, 1000])
def test_point_counts(n):
    _, stats = check_batch([_scene(7, 11, n, 40 + n, specials=False)])
    assert stats[0, 0] == n


@pytest.mark.parametrize("vel_depth", [False, True])
def test_contention_on_one_pixel(vel_depth):
    """600 points on pixel (1, 2) of a 3 x 5 map, more than a workgroup, with depths that tie (x on a lattice of 8 values), behind
    one point on another pixel: the pixel takes the group's minimum, whoever arrives first."""
    g = np.random.default_rng(9)
    x = (2.0 + g.integers(0, 8, 600)).astype(np.float32)
    crowd = np.stack([x, 3 * x, 2 * x, np.ones_like(x)], 1)                  # u = rint(3) - 1 = 2, v = rint(2) - 1 = 1
    points = np.concatenate([np.array([[4.0, 4.0, 4.0, 1.0]], np.float32), crowd], 0)
    gt, stats = check_batch([(points, velo_util.PERMUTE, 3, 5)], vel_depth)
    assert stats[0].tolist() == [601, 0, 0, 601, 2, 0] and gt[0, 1, 2] == x.min() and gt[0, 0, 0] == 4.0


def test_unaligned_base_pointer():
    """The points start four bytes into an allocation: no 16-byte load fits them."""
    frames = [_scene(9, 14, 400, 1), _scene(12, 33, 1000, 2)]
    flat = np.concatenate([f[0] for f in frames], 0).reshape(-1)
    buffer = torch.zeros(flat.size + 4, dtype=torch.float32, device=_dev())
    buffer[1:1 + flat.size] = _d(flat)
    view = buffer[1:1 + flat.size].view(-1, 4)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    check_batch(frames, points_d=view)


@pytest.mark.parametrize("name", sorted(velo_util.hand_cases()))
def test_hand_made_cases(name):
    case = velo_util.hand_cases()[name]
    gt, stats = check_batch([case[:4]], case[4])
    want, want_stats = velo_util.hand_expected(case)
    assert np.array_equal(gt[0], want.astype(np.float32)) and np.array_equal(stats[0], want_stats)


def test_hand_made_cases_as_one_batch():
    cases = [c for c in velo_util.hand_cases().values() if not c[4]]
    check_batch([c[:4] for c in cases])


def test_two_calls_return_the_same_bits():
    frames = [_scene(12, 33, 3000, 2), _scene(9, 14, 400, 1)]
    workspace = velodyne.velo_workspace(4, 16, 40, _dev())                  # larger than needed, reused between the calls
    a = run_batch(frames, workspace=workspace)
    b = run_batch(frames, workspace=workspace)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])


def test_a_size_the_tables_cannot_hold_is_reported():
    """sizes live on the device, so the host cannot refuse them: the frame's map is zero and its stats row is -1."""
    good = _scene(9, 14, 400, 1)
    points = _d(good[0])
    offsets, P = _d(np.array([0, 400, 400], np.int64)), _d(np.stack([good[1], good[1]], 0))
    gt, stats = velodyne.depth_maps_hip(points, offsets, P, _d(np.array([[9, 14], [9, 1]], np.int32)), max_size=(9, 14))
    want, want_stats = velodyne.depth_map_numpy(*good)
    assert np.array_equal(gt[0].cpu().numpy(), want.astype(np.float32)) and np.array_equal(stats[0].cpu().numpy(), want_stats)
    assert not gt[1].any() and stats[1].tolist() == [-1] * 6


def test_refusals():
    frame = _scene(9, 14, 400, 1)
    points, offsets = _d(frame[0]), _d(np.array([0, 400], np.int64))
    P, sizes = _d(frame[1][None]), _d(np.array([[9, 14]], np.int32))
    with pytest.raises(native.NativeLibraryError):                          # a CPU tensor
        velodyne.depth_maps_hip(points.cpu(), offsets, P, sizes)
    with pytest.raises(native.NativeLibraryError):
        velodyne.depth_maps_hip(points, offsets, P, sizes.cpu(), max_size=(9, 14))
    small = torch.empty(velodyne.velo_workspace(1, 9, 14, _dev()).numel() - 8, dtype=torch.uint8, device=_dev())
    with pytest.raises(native.NativeLibraryError):                          # a workspace that is too small
        velodyne.depth_maps_hip(points, offsets, P, sizes, workspace=small)
    with pytest.raises(ValueError):
        velodyne.depth_maps_hip(points, offsets, P.float(), sizes)
    # the C entry: -1 before any launch
    lib = native.load()
    ws = velodyne.velo_workspace(1, 9, 14, _dev())
    gt = torch.empty(1, 9, 14, device=_dev())
    stats = torch.full((1, 6), 77, dtype=torch.int64, device=_dev())
    ok = [native.ptr(points), native.ptr(offsets), 1, native.ptr(P), native.ptr(sizes), 9, 14, 0, native.ptr(ws), ws.numel(),
          native.ptr(gt), native.ptr(stats), native.stream()]
    for pos, bad in ((0, None), (1, None), (3, None), (4, None), (8, None), (10, None), (11, None), (2, 0), (6, 1), (9, ws.numel() - 8)):
        args = list(ok)
        args[pos] = bad
        assert lib.td_velo_depth(*args) == -1, (pos, bad)
    torch.cuda.synchronize()
    assert bool((stats == 77).all())                                        # nothing was launched
    assert lib.td_velo_depth(*ok) == 0


def test_evaluator_end_to_end(tmp_path):
    """DepthEvaluator on a tiny raw KITTI tree: two frames, two calibration dates, ground truth of two sizes.  The rows under
    gt_source = "velodyne" (td_velo_depth per batch) equal, bit for bit, the rows from the archive that export_gt_depth wrote for the
    same frames on the device.  The frames are resized to 64 x 128, the smallest the depth network runs at (below it its 1/32 level
    is a single row, which the reflection padding refuses)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import export_gt_depth
    finally:
        sys.path.pop(0)
    from mmcv import ConfigDict
    from mono.datasets.kitti_dataset import KITTIRAWDataset
    from tests.infer_util import build_model
    from tripled_amd.evaluate import DepthEvaluator
    root = str(tmp_path)
    lines, truth = velo_util.make_kitti_tree(root)
    out = os.path.join(root, "gt_depths.npz")
    data, sizes = export_gt_depth.export(root, lines, out, device=_dev())
    assert len({tuple(s) for s in sizes}) == 2
    for i, line in enumerate(lines):                                        # the device export is the statement
        points, calib = truth[line]
        H, W = velo_util.size_of(calib)
        want = velodyne.depth_map_numpy(points, velo_util.projection(calib, 2 if line.split()[2] == "l" else 3), H, W)[0]
        assert np.array_equal(_bits(data[i, :H, :W]), _bits(want.astype(np.float32)))

    def dataset(**cfg):
        path = cfg.pop("gt_depth_path", None)
        return KITTIRAWDataset(root, lines, 64, 128, [0], is_train=False, img_ext=".png", gt_depth_path=path, cfg=ConfigDict(**cfg))

    from mono.datasets import collate_validation
    from tripled_amd import evaluate, infer
    model = build_model("cfg_kitti_fm", 32, 64).to(_dev()).eval()
    ev = DepthEvaluator(model, _dev(), batch_size=2)
    from_scans, from_archive = dataset(gt_source="velodyne"), dataset(gt_depth_path=out)
    samples_v, samples_a = [from_scans[i] for i in range(2)], [from_archive[i] for i in range(2)]
    # the evaluator's ground truth of the batch: the same padded tensors, bit for bit
    built = ev.ground_truth(samples_v)
    padded = evaluate.pad_ground_truth(ev.ground_truth(samples_a), _dev())
    assert isinstance(built, tuple) and built[0].shape == (2, 30, 52)
    for mine, theirs in zip(built, padded):
        assert mine.dtype == theirs.dtype and mine.shape == theirs.shape
        assert np.array_equal(mine.cpu().numpy().view(np.uint32), theirs.cpu().numpy().view(np.uint32))
    # the rows of ONE forward pass scored against both (two passes of the convolution library need not return the same bits, which
    # would say nothing about the ground truth)
    net, restore = infer.eval_network(model, _dev(), "fp32")
    with torch.no_grad(), restore:
        disp = ev._forward(net, collate_validation(samples_v, _dev()))
        rows_v, counts_v = ev.score(disp, built)
        rows_a, counts_a = ev.score(disp, [s["gt_depth"] for s in samples_a])
    rows_v, rows_a = rows_v.cpu().numpy(), rows_a.cpu().numpy()
    assert int(counts_v.min()) > 0 and torch.equal(counts_v, counts_a)
    assert np.array_equal(rows_v.view(np.uint32), rows_a.view(np.uint32))
    # and through evaluate_rows, each with its own forward pass: the same frames scored, the rows within the evaluation tests' bound
    # for a forward pass (tests/eval_util.py: relative 1e-5)
    full_v, n_v = ev.evaluate_rows(from_scans)
    full_a, n_a = ev.evaluate_rows(from_archive)
    assert np.array_equal(n_v, n_a) and np.array_equal(n_v, counts_v.cpu().numpy())
    print("evaluate_rows, scans against archive: max relative difference %.3e" % float(np.max(np.abs(full_v - full_a) / np.abs(full_a))))
    np.testing.assert_allclose(full_v, full_a, rtol=1e-5, atol=0)
    np.testing.assert_allclose(full_v, rows_v, rtol=1e-5, atol=0)
