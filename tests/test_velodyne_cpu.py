"""tripled_amd.velodyne on the host: the numpy statement of the reference's generate_depth_map against a literal per-point loop,
against the reference's recorded maps (tests/golden/velodyne.npz, tools/gen_golden_velo.py) and against maps written down by hand
for every rule; the pickle-free archive, KITTIRAWDataset.get_depth and the validation sample's keys.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tests import velo_util
from tripled_amd import native, velodyne

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "velodyne.npz")
# the statement's four-term sums are rounded term by term, np.dot's through BLAS: the allowance test_odometry_cpu.py gives for
# "another BLAS rounds a product differently"
BLAS_RTOL = 1e-12


def golden_scenes():
    """[(name, calibration dict, points, {(cam, vel_depth): the reference's map})]"""
    g = np.load(GOLDEN)
    out = []
    for name, H, W, n, _ in velo_util.GOLDEN_SCENES:
        calib = {k: g["%s_%s" % (name, k)] for k in velo_util.CALIB_KEYS}
        maps = {(cam, vd): g["%s_depth_cam%d_vel%d" % (name, cam, int(vd))] for cam in (2, 3) for vd in (False, True)}
        assert velo_util.size_of(calib) == (H, W) and g[name + "_points"].shape == (n, 4)
        out.append((name, calib, g[name + "_points"], maps))
    return out


def check_against_reference(mine, ref, vel_depth, what):
    """The rule for a map against the reference's: vel_depth copies x, so every pixel is equal; otherwise the zero pattern is
    equal and the values agree within BLAS_RTOL."""
    assert mine.shape == ref.shape and mine.dtype == np.float64, what
    if vel_depth:
        assert np.array_equal(mine, ref), what
        return
    assert np.array_equal(mine == 0, ref == 0), what
    nz = ref != 0
    err = float(np.max(np.abs(mine[nz] - ref[nz]) / np.abs(ref[nz]))) if nz.any() else 0.0
    print("%s: relative error %.3e over %d pixels" % (what, err, int(nz.sum())))
    assert err <= BLAS_RTOL, what


@pytest.mark.parametrize("vel_depth", [False, True])
def test_statement_equals_bruteforce(vel_depth):
    for name, calib, points, _ in golden_scenes():
        H, W = velo_util.size_of(calib)
        for cam in (2, 3):
            P = velo_util.projection(calib, cam)
            m, s = velodyne.depth_map_numpy(points, P, H, W, vel_depth)
            mb, sb = velodyne.depth_map_bruteforce(points, P, H, W, vel_depth)
            assert np.array_equal(m, mb) and np.array_equal(s, sb), (name, cam, s, sb)
            assert s[0] == len(points) and s[1] + s[2] + s[3] == s[0]
            # a pixel that was hit is non-zero or was clamped, except at d = x = 0 exactly, which only vel_depth can give
            assert s[4] >= np.count_nonzero(m) + s[5] and (vel_depth or s[4] == np.count_nonzero(m) + s[5])
    # other sizes and point counts, without the special points too
    for H, W, n, seed in ((2, 2, 40, 3), (5, 7, 257, 4), (17, 3, 1000, 5)):
        calib = velo_util.synthetic_calibration(H, W, seed)
        points = velo_util.synthetic_scan(calib, n, seed, specials=seed != 4)
        P = velo_util.projection(calib, 2)
        m, s = velodyne.depth_map_numpy(points, P, H, W, vel_depth)
        mb, sb = velodyne.depth_map_bruteforce(points, P, H, W, vel_depth)
        assert np.array_equal(m, mb) and np.array_equal(s, sb), (H, W, n)


def test_statement_against_golden():
    for name, calib, points, maps in golden_scenes():
        H, W = velo_util.size_of(calib)
        for (cam, vd), ref in maps.items():
            m, _ = velodyne.depth_map_numpy(points, velo_util.projection(calib, cam), H, W, vd)
            check_against_reference(m, ref, vd, "scene %s cam %d vel_depth %d" % (name, cam, vd))


def test_golden_exercises_the_rules():
    for name, calib, points, maps in golden_scenes():
        H, W = velo_util.size_of(calib)
        P = velo_util.projection(calib, 2)
        mixed, dups = velo_util.false_collisions(points, P, H, W)
        stats = dict(zip(velodyne.STATS, velodyne.depth_map_numpy(points, P, H, W)[1]))
        assert dups > 0 and mixed > 0, name
        assert stats["pixels_clamped"] > 0 and stats["behind"] > 0 and stats["outside"] > 0 and stats["valid"] > stats["pixels_hit"], stats
        assert float(maps[(2, False)].min()) == 0.0             # the reference clamped it too


@pytest.mark.parametrize("name", sorted(velo_util.hand_cases()))
def test_hand_made_cases(name):
    case = velo_util.hand_cases()[name]
    want, want_stats = velo_util.hand_expected(case)
    for fn in (velodyne.depth_map_numpy, velodyne.depth_map_bruteforce):
        m, s = fn(*case[:5])
        assert np.array_equal(m, want), (name, fn.__name__, m)
        assert np.array_equal(s, want_stats), (name, fn.__name__, s)


def test_ordered_bits():
    d = np.array([-np.inf, -3.5, -1e-300, -0.0, 0.0, 1e-300, 2.0, np.inf])
    k = velodyne.ordered_bits(d)
    assert np.all(k[1:] > k[:-1])
    assert np.array_equal(velodyne.from_ordered_bits(k).view(np.uint64), d.view(np.uint64))


def test_bad_arguments():
    pts = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError):
        velodyne.depth_map_numpy(pts, np.eye(4), 4, 4)
    with pytest.raises(ValueError):
        velodyne.depth_map_numpy(pts, velo_util.PERMUTE, 4, 1)          # W - 1 = 0 would join every column
    with pytest.raises(ValueError):
        velodyne.depth_map_numpy(np.zeros((3, 3), np.float32), velo_util.PERMUTE, 4, 4)
    with pytest.raises(native.NativeLibraryError):                      # the kernel path never runs on host tensors
        velodyne.depth_maps_hip(torch.zeros(3, 4), torch.tensor([0, 3]), torch.zeros(1, 3, 4, dtype=torch.float64),
                                torch.tensor([[4, 4]], dtype=torch.int32))


def test_c_entry_refuses_without_a_launch():
    lib = native.load()
    assert lib.td_velo_depth_workspace_bytes(0, 8, 8) == 0 and lib.td_velo_depth_workspace_bytes(1, 8, 1) == 0
    # one 64-bit entry per pixel and three per group
    assert lib.td_velo_depth_workspace_bytes(3, 9, 14) == 3 * (9 * 14 + 3 * (9 * 13 + 1)) * 8
    assert lib.td_velo_depth_workspace_bytes(12, 376, 1242) == 12 * (376 * 1242 + 3 * (376 * 1241 + 1)) * 8
    assert lib.td_velo_depth(None, None, 1, None, None, 8, 8, 0, None, 0, None, None, None) == -1
    ok = [0x1000, 0x2000, 1, 0x3000, 0x4000, 8, 8, 0, 0x5000, 1 << 20, 0x6000, 0x7000, None]      # never dereferenced on the host
    for pos in (0, 1, 3, 4, 8, 10, 11):
        args = list(ok)
        args[pos] = None
        assert lib.td_velo_depth(*args) == -1, pos
    for pos, bad in ((2, 0), (2, -1), (5, 0), (6, 1), (9, 8)):                                     # B, Hmax, Wmax < 2, a small workspace
        args = list(ok)
        args[pos] = bad
        assert lib.td_velo_depth(*args) == -1, (pos, bad)


def test_calibration_files(tmp_path):
    for name, calib, _, _ in golden_scenes():
        d = str(tmp_path / name)
        velo_util.write_calib(d, calib)
        read = velodyne.read_calib_file(os.path.join(d, "calib_cam_to_cam.txt"))
        assert isinstance(read["calib_time"], str) and read["corner_dist"].shape == (1,)
        for k in ("S_rect_02", "P_rect_02", "P_rect_03", "R_rect_00"):
            assert np.array_equal(read[k], calib[k]), k
        for cam in (2, 3):
            P, size = velodyne.velo_to_image(d, cam)
            assert np.array_equal(P, velo_util.projection(calib, cam)) and size == velo_util.size_of(calib)      # S_rect_02 for camera 3 too


def test_scan_file(tmp_path):
    pts = velo_util.synthetic_scan(velo_util.synthetic_calibration(9, 14, 1), 100, 7)
    path = velo_util.write_scan(str(tmp_path), "d/drive", 3, pts)
    got = velodyne.load_velodyne_points(path)
    assert got.dtype == np.float32 and got.shape == (100, 4)
    assert np.array_equal(got[:, :3], pts[:, :3], equal_nan=True) and np.all(got[:, 3] == 1.0)


def _dataset(root, lines, height=24, width=40, **data_cfg):
    from mmcv import ConfigDict
    from mono.datasets.kitti_dataset import KITTIRAWDataset
    gt_path = data_cfg.pop("gt_depth_path", None)
    return KITTIRAWDataset(root, lines, height, width, [0], is_train=False, img_ext=".png", gt_depth_path=gt_path, cfg=ConfigDict(**data_cfg))


def _expected_map(truth, line):
    points, calib = truth[line]
    cam = 2 if line.split()[2] == "l" else 3
    H, W = velo_util.size_of(calib)
    return velodyne.depth_map_numpy(points, velo_util.projection(calib, cam), H, W)[0].astype(np.float32)


def test_get_depth(tmp_path):
    lines, truth = velo_util.make_kitti_tree(str(tmp_path))
    ds = _dataset(str(tmp_path), lines)
    assert ds.check_depth()
    for line in lines:
        folder, frame_index, side = line.split()
        want = _expected_map(truth, line)
        got = ds.get_depth(folder, int(frame_index), side, False)
        assert got.dtype == np.float32 and np.array_equal(got, want) and np.count_nonzero(got) > 20
        assert np.array_equal(ds.get_depth(folder, int(frame_index), side, True), np.fliplr(want))


def test_velodyne_samples_and_collate(tmp_path):
    from mono.datasets import collate_validation
    lines, truth = velo_util.make_kitti_tree(str(tmp_path))
    ds = _dataset(str(tmp_path), lines, gt_source="velodyne")
    samples = [ds[i] for i in range(len(ds))]
    for s, line in zip(samples, lines):
        points, calib = truth[line]
        assert "gt_depth" not in s and s["velo"].dtype == torch.float32 and s["velo_P"].dtype == torch.float64
        assert np.array_equal(s["velo"].numpy()[:, :3], points[:, :3], equal_nan=True)
        assert tuple(int(v) for v in s["gt_size"]) == velo_util.size_of(calib) and s["gt_size"].dtype == torch.int32
        assert np.array_equal(velodyne.sample_ground_truth(s), _expected_map(truth, line))
    batch = collate_validation(samples, "cpu")                          # scans of different lengths: they must not be stacked
    assert not any(k in batch for k in ("velo", "velo_P", "gt_size", "gt_depth"))
    assert batch[("color", 0, 0)].shape == (len(lines), 3, 24, 40)
    # the default is unchanged: no archive, no ground truth in the sample
    plain = _dataset(str(tmp_path), lines)[0]
    assert not any(k in plain for k in ("velo", "velo_P", "gt_size", "gt_depth"))
    # the host batches of the loader and of the evaluator
    maps = velodyne.VelodyneGroundTruth(str(tmp_path), "cpu")([tuple(line.split()) for line in lines])
    for m, line in zip(maps, lines):
        assert m.dtype == np.float32 and np.array_equal(m, _expected_map(truth, line))


def test_archive_round_trip(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import export_gt_depth
    finally:
        sys.path.pop(0)
    lines, truth = velo_util.make_kitti_tree(str(tmp_path), frames_per_drive=2)
    out = str(tmp_path / "gt_depths.npz")
    data, sizes = export_gt_depth.export(str(tmp_path), lines, out, device="cpu", batch_size=3)
    with np.load(out, allow_pickle=False) as archive:                   # pickle-free
        assert sorted(archive.files) == ["data", "sizes"]
        assert archive["data"].dtype == np.float32 and archive["sizes"].dtype == np.int32
        assert archive["data"].shape == (4, 30, 52) and np.array_equal(archive["data"], data)
    ds = _dataset(str(tmp_path), lines, gt_depth_path=out)
    for i, line in enumerate(lines):
        want = _expected_map(truth, line)
        got = ds[i]["gt_depth"]
        assert got.shape == want.shape and np.array_equal(got, want)
        h, w = sizes[i]
        assert not data[i, h:].any() and not data[i, :, w:].any()      # the padding is zero
    assert len({tuple(s) for s in sizes}) == 2
    # gt_source = "velodyne" wins over an archive that is also configured
    assert "velo" in _dataset(str(tmp_path), lines, gt_depth_path=out, gt_source="velodyne")[0]


def test_archive_without_sizes_loads_as_before(tmp_path):
    lines, _ = velo_util.make_kitti_tree(str(tmp_path))
    data = np.random.default_rng(0).uniform(1, 50, (2, 11, 13)).astype(np.float32)
    out = str(tmp_path / "plain.npz")
    np.savez(out, data=data)
    ds = _dataset(str(tmp_path), lines, gt_depth_path=out)
    assert ds.gt_sizes is None
    for i in range(2):
        assert np.array_equal(ds[i]["gt_depth"], data[i])


def test_evaluator_on_the_host_scores_velodyne_samples(tmp_path):
    """DepthEvaluator on 'cpu': samples that carry a scan score like samples that carry the exported archive's map.  The frames
    are resized to 64 x 128, the smallest the depth network runs at (below it the 1/32 level is a single row, which the reflection
    padding refuses); the ground truths keep their own two sizes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import export_gt_depth
    finally:
        sys.path.pop(0)
    from tests.infer_util import build_model
    from tripled_amd.evaluate import DepthEvaluator
    lines, _ = velo_util.make_kitti_tree(str(tmp_path))
    out = str(tmp_path / "gt_depths.npz")
    export_gt_depth.export(str(tmp_path), lines, out, device="cpu")
    model = build_model("cfg_kitti_fm", 32, 64).eval()
    ev = DepthEvaluator(model, "cpu", batch_size=2)
    rows_v, counts_v = ev.evaluate_rows(_dataset(str(tmp_path), lines, 64, 128, gt_source="velodyne"))
    rows_a, counts_a = ev.evaluate_rows(_dataset(str(tmp_path), lines, 64, 128, gt_depth_path=out))
    assert np.array_equal(rows_v, rows_a) and np.array_equal(counts_v, counts_a) and counts_v.min() > 0
