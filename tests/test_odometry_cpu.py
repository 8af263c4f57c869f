"""tripled_amd.odometry on the host: the numpy statements against the reference's recorded numbers (tests/golden/odometry.npz,
tools/gen_golden_pose.py), the pose text round trip, KITTIOdomDataset, OdometryEvaluator(device='cpu') and the argument checks of
the four td_* entry points.  Bounds: tests/odom_util.py."""
import os

import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import native, odometry
from tests import odom_util as U
from tests.infer_util import build_model


def test_snippet_ates_are_the_references():
    g = U.golden()
    ates = odometry.snippet_ates_numpy(g["rel"], g["gt"])
    assert ates.shape == (299,) and U.rel_err(ates, g["ates"]) <= U.RTOL
    # the short snippets at the end divide by their own point count: entry n-1 has two points
    assert U.rel_err(odometry.snippet_ates_numpy(g["rel"][-1:], g["gt"][-2:]), g["ates"][-1:]) <= U.RTOL


def test_trajectory_is_the_references():
    g = U.golden()
    traj = odometry.trajectory_numpy(g["rel"])
    assert traj.dtype == np.float64 and U.traj_err(traj, g["traj"]) <= U.RTOL
    assert np.array_equal(traj[0], np.eye(4)[:3])


def test_sequence_errors_are_the_toolkits():
    g = U.golden()
    lengths = [int(v) for v in g["lengths"]]
    rows, scale, distance = odometry.sequence_errors_numpy(g["gt"], g["traj"], lengths)
    assert rows.shape == g["seq_err"].shape                                   # the same rows in the same order
    for col in (0, 3, 4):                                                     # first_frame, len, speed: exact
        assert np.array_equal(rows[:, col], g["seq_err"][:, col]), col
    assert U.rel_err(rows[:, 1:3], g["seq_err"][:, 1:3]) <= U.RTOL
    assert abs(scale - float(g["scale"])) <= U.RTOL * float(g["scale"]) and 20 < scale < 50        # 1 / 0.03
    assert distance == float(g["distance"])                                   # sequential sum: bit-identical
    assert U.rel_err(np.array(odometry.overall_errors(rows)), g["overall"]) <= U.RTOL
    seg = odometry.segment_errors(rows, lengths)
    assert U.rel_err(np.array([[k] + seg[k] for k in lengths]), g["segment"]) <= U.RTOL
    assert odometry.segment_errors(rows, [100, 300])[300] == []
    assert abs(odometry.umeyama_scale_numpy(g["traj"][:, :, 3], g["gt"][:, :, 3]) - float(g["scale"])) <= U.RTOL * float(g["scale"])
    unscaled, one, _ = odometry.sequence_errors_numpy(g["gt"], g["traj"], lengths, align_scale=False)
    assert one == 1.0 and np.array_equal(unscaled[:, 0], rows[:, 0]) and float(unscaled[:, 2].min()) > float(rows[:, 2].max())
    assert np.all(np.isnan(odometry.overall_errors(np.zeros((0, 5)))))


def test_fixture_is_well_conditioned():
    g = U.golden()
    lengths = [int(v) for v in g["lengths"]]
    U.assert_conditions(g["seq_err"], odometry.trajectory_distances(g["gt"]), lengths, 10)
    assert len(g["seq_err"]) > 20 and set(g["seq_err"][:, 3]) == {100.0, 200.0}


def test_kitti_pose_text_round_trip(tmp_path):
    g = U.golden()
    path = str(tmp_path / "09_pred.txt")
    odometry.save_kitti_poses(path, g["traj"])
    lines = open(path).read().splitlines()
    assert len(lines) == 300 and all(len(l.split()) == 12 for l in lines) and lines[0].split()[0] == "1.00000000e+00"
    back = odometry.load_kitti_poses(path)
    assert back.shape == (300, 3, 4) and back.dtype == np.float64
    assert np.all(np.abs(back - g["traj"]) <= 5.0000001e-9 * np.abs(g["traj"]))                      # %1.8e: 9 significant digits
    odometry.save_kitti_poses(path, back)
    assert np.array_equal(odometry.load_kitti_poses(path), back)                                   # text -> text is exact
    one = str(tmp_path / "one.txt")
    odometry.save_kitti_poses(one, g["traj"][:1])
    assert odometry.load_kitti_poses(one).shape == (1, 3, 4)


def test_pairs_torch():
    frames = torch.arange(3 * 3 * 2 * 5, dtype=torch.int64).remainder(256).to(torch.uint8).reshape(3, 3, 2, 5)
    pairs = odometry.pairs_torch(frames)
    assert pairs.shape == (2, 6, 2, 5) and pairs.dtype == torch.float32
    assert torch.equal(pairs[1, :3], frames[1].float() / 255.0) and torch.equal(pairs[1, 3:], frames[2].float() / 255.0)
    with pytest.raises(ValueError):
        odometry.pairs_torch(frames.float())


def test_odometry_dataset_paths_and_lines(tmp_path):
    import mono.datasets
    from mono.datasets import KITTIOdomDataset, odom_sequence_files
    from mono.datasets.get_dataset import get_dataset
    U.make_sequence_tree(str(tmp_path), 9, 3, h=40, w=72)
    files = odom_sequence_files(9, 3)
    assert files == ["9 0 l", "9 1 l"] and odom_sequence_files("10", 1201)[-1] == "10 1199 l"
    with pytest.raises(ValueError):
        odom_sequence_files(9, 1)
    ds = KITTIOdomDataset(str(tmp_path), files, 32, 64, [0, 1], is_train=False, img_ext=".png")
    assert ds.side_map == {"l": 0, "r": 1} and len(ds) == 2
    assert ds.get_image_path("9", 7, "l") == os.path.join(str(tmp_path), "sequences/09", "image_0", "000007.png")
    assert ds.get_image_path("10", 123456, "r") == os.path.join(str(tmp_path), "sequences/10", "image_1", "123456.png")
    sample = ds[0]
    assert sample[("color", 0, 0)].shape == (3, 32, 64) and sample[("color", 1, 0)].shape == (3, 32, 64)
    assert torch.equal(ds.frame_u8(0, 1).float().div(255.0), sample[("color", 1, 0)])              # decoded once, the same frame
    assert torch.equal(ds.frame_u8(1, 0), ds.frame_u8(0, 1)) and ds.frame_u8(1, 1).dtype == torch.uint8
    frames = odometry.dataset_frames_u8(ds)
    assert frames.shape == (3, 3, 32, 64) and torch.equal(frames[2], ds.frame_u8(1, 1))
    reg = get_dataset(dict(name="kitti_odom", in_path=str(tmp_path), sequence=9, n_frames=3, height=32, width=64), training=False)
    assert isinstance(reg, KITTIOdomDataset) and reg.filenames == files
    split = tmp_path / "pairs.txt"
    split.write_text("9 1 l\n")
    reg = get_dataset(dict(name="kitti_odom", in_path=str(tmp_path), split_file=str(split), height=32, width=64), training=False)
    assert reg.filenames == ["9 1 l"]
    assert mono.datasets.KITTIOdomDataset is KITTIOdomDataset


def test_evaluator_on_the_host(tmp_path):
    from mono.datasets import KITTIOdomDataset, odom_sequence_files
    gt = U.make_sequence_tree(str(tmp_path), 9, 3)
    ds = KITTIOdomDataset(str(tmp_path), odom_sequence_files(9, 3), 32, 64, [0, 1], is_train=False, img_ext=".png")
    model = build_model("cfg_kitti_fm", 32, 64).train()
    ev = odometry.OdometryEvaluator(model, "cpu", batch_size=1)
    res = ev.evaluate(ds, gt, lengths=(0.5, 1.5), step=1)
    assert model.training and all(m.training for m in model.modules())
    rel = res.relative.numpy()
    assert rel.shape == (2, 4, 4) and rel.dtype == np.float32 and np.array_equal(rel[:, 3], np.tile([0, 0, 0, 1.0], (2, 1)))
    # the same pairs in one batch of two, and through the model's own statements
    both = odometry.OdometryEvaluator(model.eval(), "cpu", batch_size=12).relative_poses(ds)
    assert float((both - res.relative).abs().max()) < 1e-6
    with torch.no_grad():
        a, t = model.PoseDecoder(model.PoseEncoder(odometry.pairs_torch(odometry.dataset_frames_u8(ds))[:1]))
        assert torch.equal(model.transformation_from_parameters(a[:, 0], t[:, 0])[0], res.relative[0])
    assert np.array_equal(res.poses, odometry.trajectory_numpy(rel))
    assert np.array_equal(res.ates, odometry.snippet_ates_numpy(rel, gt))
    rows, scale, distance = odometry.sequence_errors_numpy(gt, res.poses, (0.5, 1.5), 1)
    assert np.array_equal(res.segments, rows) and len(rows) == 3 and res.scale == scale and res.distance == distance
    assert (res.t_err, res.r_err) == odometry.overall_errors(rows)
    assert res.ate_mean == float(np.mean(res.ates)) and res.ate_std == float(np.std(res.ates))
    with pytest.raises(ValueError):
        odometry.OdometryEvaluator(model, "cpu", precision="bf16")
    with pytest.raises(ValueError):
        ev.evaluate(ds, gt[:2])


def test_device_entry_points_refuse_host_tensors():
    with pytest.raises(native.NativeLibraryError):
        odometry.pairs_hip(torch.zeros(2, 3, 4, 8, dtype=torch.uint8))
    with pytest.raises(native.NativeLibraryError):
        odometry.trajectory_hip(torch.eye(4).repeat(2, 1, 1))
    with pytest.raises(native.NativeLibraryError):
        odometry.snippet_ates_hip(torch.eye(4).repeat(2, 1, 1), torch.zeros(3, 3, 4, dtype=torch.float64))
    with pytest.raises(native.NativeLibraryError):
        odometry.sequence_errors_hip(torch.zeros(3, 3, 4, dtype=torch.float64), torch.zeros(3, 3, 4, dtype=torch.float64))


def test_argument_validation_without_gpu():
    import ctypes
    lib = native.load()
    assert lib.td_abi_version() == 3
    lengths = (ctypes.c_double * 2)(100.0, 200.0)
    one = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: the size checks come first
    assert lib.td_pose_pairs_u8(None, 2, 8, 8, 0, 2, 0, None, 0, None) == -1
    assert lib.td_pose_pairs_u8(one, 2, 8, 8, 1, 2, 0, one, 0, None) == -1          # window past the last pair
    assert lib.td_pose_pairs_u8(one, 2, 8, 8, 0, 2, 7, one, 0, None) == -1          # unknown dtype
    assert lib.td_pose_pairs_u8(one, 2, 0, 8, 0, 2, 0, one, 0, None) == -1
    assert lib.td_odom_trajectory(None, 0, 4, None, None) == -1
    assert lib.td_odom_trajectory(one, 0, 0, one, None) == -1
    assert lib.td_odom_snippet_ate(None, 0, None, 4, 5, None, None) == -1
    assert lib.td_odom_snippet_ate(one, 0, one, 4, 1, one, None) == -1              # track_length 2 ... 16
    assert lib.td_odom_snippet_ate(one, 0, one, 4, 17, one, None) == -1
    assert lib.td_odom_sequence_errors(None, None, 4, lengths, 2, 10, 1, None, None, None, None, None) == -1
    assert lib.td_odom_sequence_errors(one, one, 4, lengths, 17, 10, 1, one, one, one, one, None) == -1
    assert lib.td_odom_sequence_errors(one, one, 4, lengths, 2, 0, 1, one, one, one, one, None) == -1
    assert lib.td_odom_sequence_errors(one, one, 4, None, 2, 10, 1, one, one, one, one, None) == -1
    assert lib.td_odom_sequence_errors(one, one, 4, (ctypes.c_double * 2)(100.0, -1.0), 2, 10, 1, one, one, one, one, None) == -1


def test_no_plotting_dependency():
    """No plots: neither the module nor the script names matplotlib (the reference's toolkit imports it at the top)."""
    for path in (odometry.__file__, os.path.join(U.ROOT, "scripts", "eval_pose.py")):
        assert "import matplotlib" not in open(path).read() and "from matplotlib" not in open(path).read(), path
