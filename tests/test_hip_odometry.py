"""csrc/td_odom.hip on the device (through tripled_amd.odometry): the pairs bit for bit against pairs_torch, the trajectory scan, the
snippet ATE and the segment errors against the float64 host statements (and the reference's recorded numbers), then
OdometryEvaluator and scripts/eval_pose.py on a six-frame tree.  Bounds and input conditions: tests/odom_util.py (1e-9 relative,
derived from the float64 rounding of <= 4 540 compositions; first_frame, len, validity and row count exact)."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import odometry
from tests import odom_util as U
from tests.infer_util import build_model, randomize_batchnorm

pytestmark = pytest.mark.gpu

T = odometry.TRAJECTORY_THREADS
_cache = {}


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_on_the_device():
    """The cached model and tensors go when the module is done, as in test_hip_eval.py."""
    yield
    _cache.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


# ---- 1. pairs ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,h,w", [(2, 5, 7), (2, 8, 32), (4, 8, 16), (3, 192, 640)])
def test_pairs_are_totensor_and_cat(n, h, w):
    g = torch.Generator().manual_seed(n * h)
    frames = torch.randint(0, 256, (n + 1, 3, h, w), generator=g, dtype=torch.uint8)
    frames[0, 0, 0, :5] = torch.tensor([0, 1, 127, 128, 255], dtype=torch.uint8)
    frames.view(-1)[-256:] = torch.arange(256, dtype=torch.int64).to(torch.uint8)      # every byte value, in the scalar path too
    want = odometry.pairs_torch(frames)
    got = odometry.pairs_hip(frames.to(_dev()))
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)
    got16 = odometry.pairs_hip(frames.to(_dev()), torch.bfloat16)
    assert got16.dtype == torch.bfloat16 and torch.equal(got16.cpu(), want.to(torch.bfloat16))
    if n >= 3:
        # a window in the middle: the other rows are left alone
        for dtype in (torch.float32, torch.bfloat16):
            out = torch.full((n, 6, h, w), -7.0, dtype=dtype, device=_dev())
            assert odometry.pairs_hip(frames.to(_dev()), dtype, first=1, count=n - 2, out=out) is out
            ref = torch.full((n, 6, h, w), -7.0, dtype=dtype)
            ref[1:n - 1] = want[1:n - 1].to(dtype)
            assert torch.equal(out.cpu(), ref)
        # the same window into a batch buffer
        batch = torch.full((n, 6, h, w), -7.0, device=_dev())
        odometry.pairs_hip(frames.to(_dev()), first=1, count=n - 2, out=batch, out_first=0)
        assert torch.equal(batch[:n - 2].cpu(), want[1:n - 1]) and bool((batch[n - 2:] == -7.0).all())
    with pytest.raises(ValueError):
        odometry.pairs_hip(frames.to(_dev()), first=n - 1, count=2)


# ---- 2. trajectory -----------------------------------------------------------------------------------------------------------------

def _trajectory_case(n, dtype=np.float32):
    key = ("traj", n, np.dtype(dtype).name)
    if key not in _cache:
        rel = U.smooth_relative(n, seed=n, dtype=dtype)
        _cache[key] = (rel, odometry.trajectory_numpy(rel))
    return _cache[key]


@pytest.mark.parametrize("n", [1, 2, T - 1, T, T + 1, 1590, 4540])
def test_trajectory_scan(n):
    rel, want = _trajectory_case(n)
    got = odometry.trajectory_hip(_d(rel))
    again = odometry.trajectory_hip(_d(rel))
    assert got.shape == (n + 1, 3, 4) and got.dtype == torch.float64
    err = U.traj_err(got.cpu().numpy(), want)
    print("n = %d: %.3e of max(1, max |t| = %.1f)" % (n, err, np.abs(want[:, :, 3]).max()))
    assert err <= U.RTOL
    assert torch.equal(got, again)                                            # bit-reproducible
    assert np.array_equal(got[0].cpu().numpy(), np.eye(4)[:3])


def test_trajectory_float64_input_and_long_sequence():
    rel, want = _trajectory_case(T + 7, np.float64)
    assert U.traj_err(odometry.trajectory_hip(_d(rel)).cpu().numpy(), want) <= U.RTOL
    g = U.golden()
    assert U.traj_err(odometry.trajectory_hip(_d(g["rel"])).cpu().numpy(), g["traj"]) <= U.RTOL
    # n = 8 192: composing the host's relative steps of the device's trajectory gives the input back (no host loop of 8 192)
    rel = U.smooth_relative(8192, seed=5, dtype=np.float64)
    poses = odometry.trajectory_hip(_d(rel)).cpu().numpy()
    G = np.zeros((8193, 4, 4))
    G[:, :3], G[:, 3, 3] = poses, 1.0
    back = np.linalg.inv(np.linalg.inv(G[:-1]) @ G[1:])
    assert np.abs(back - rel).max() <= U.RTOL * max(1.0, np.abs(poses[:, :, 3]).max())


# ---- 3. snippet ATE ----------------------------------------------------------------------------------------------------------------

def _ate_inputs(n, seed):
    gt = odometry.trajectory_numpy(U.smooth_relative(n, seed, dtype=np.float64))
    pred = U.smooth_relative(n, seed, bias=2e-3, scale=0.03)                 # the same motion, drifting, in the network's unit
    pred[:, :3, 3] += np.random.default_rng(seed).normal(0, 2e-3, (n, 3)).astype(np.float32)
    return pred, gt


@pytest.mark.parametrize("n,track_length", [(1, 5), (3, 5), (4, 5), (5, 5), (257, 5), (40, 2), (40, 16)])
def test_snippet_ate(n, track_length):
    pred, gt = _ate_inputs(n, seed=n + track_length)
    want = odometry.snippet_ates_numpy(pred, gt, track_length)
    got = odometry.snippet_ates_hip(_d(pred), _d(gt), track_length).cpu().numpy()
    assert got.shape == (n,) and U.rel_err(got, want) <= U.RTOL and np.all(want > 0)
    # the last track_length - 2 snippets are the short ones: entry i is the ATE of the sequence's tail on its own
    for i in range(max(0, n - (track_length - 2)), n):
        assert U.rel_err(got[i:i + 1], odometry.snippet_ates_numpy(pred[i:], gt[i:], track_length)[:1]) <= U.RTOL
    got64 = odometry.snippet_ates_hip(_d(pred.astype(np.float64)), _d(gt), track_length)
    assert np.array_equal(got64.cpu().numpy(), got)                           # float32 is widened exactly


def test_snippet_ate_golden_and_nan():
    g = U.golden()
    got = odometry.snippet_ates_hip(_d(g["rel"]), _d(g["gt"])).cpu().numpy()
    assert U.rel_err(got, g["ates"]) <= U.RTOL
    zero = np.zeros((6, 4, 4), np.float32)
    want = odometry.snippet_ates_numpy(zero, g["gt"][:7])
    assert np.all(np.isnan(want))                                             # 0 / 0, as numpy
    assert np.all(np.isnan(odometry.snippet_ates_hip(_d(zero), _d(g["gt"][:7])).cpu().numpy()))
    with pytest.raises(ValueError):
        odometry.snippet_ates_hip(_d(zero), _d(g["gt"][:7]), 17)


# ---- 4. sequence errors ------------------------------------------------------------------------------------------------------------

def _check_sequence(gt, pred, lengths, step, align):
    want_rows, want_scale, want_dist = odometry.sequence_errors_numpy(gt, pred, lengths, step, align)
    U.assert_conditions(want_rows, odometry.trajectory_distances(gt), lengths, step)
    first = odometry.sequence_errors_hip(_d(gt), _d(pred), lengths, step, align)
    again = odometry.sequence_errors_hip(_d(gt), _d(pred), lengths, step, align)
    assert all(np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True) for a, b in zip(first, again))      # bit-reproducible
    rows, valid, summary = first
    F = odometry.num_first_frames(len(gt), step)
    assert rows.shape == (F, len(lengths), 5) and valid.shape == (F, len(lengths)) and valid.dtype == torch.uint8
    rows, valid, summary = rows.cpu().numpy(), valid.cpu().numpy(), summary.cpu().numpy()
    # validity = the host's -1 cases: a (first_frame, length) is valid exactly when the host kept its row
    kept = {(int(r[0]), float(r[3])) for r in want_rows}
    for f in range(F):
        for l, length in enumerate(lengths):
            assert bool(valid[f, l]) == ((f * step, float(length)) in kept), (f, length)
            assert rows[f, l, 0] == f * step and rows[f, l, 3] == length
    assert np.all(np.isnan(rows[valid == 0][:, [1, 2, 4]]))                   # invalid, not zero
    got = odometry.compact_rows(rows, valid)
    assert got.shape == want_rows.shape
    if len(got):
        assert np.array_equal(got[:, [0, 3, 4]], want_rows[:, [0, 3, 4]])     # first_frame, len, speed: exact
        assert U.rel_err(got[:, 1:3], want_rows[:, 1:3]) <= U.RTOL
    assert abs(summary[0] - want_scale) <= U.RTOL * abs(want_scale) and summary[1] == want_dist
    return got, summary


@pytest.mark.parametrize("align", [True, False])
def test_sequence_errors_golden(align):
    g = U.golden()
    lengths = [int(v) for v in g["lengths"]]
    got, summary = _check_sequence(g["gt"], g["traj"], lengths, 10, align)
    if align:
        assert U.rel_err(got[:, 1:3], g["seq_err"][:, 1:3]) <= U.RTOL and np.array_equal(got[:, [0, 3, 4]], g["seq_err"][:, [0, 3, 4]])
        assert abs(summary[0] - float(g["scale"])) <= U.RTOL * float(g["scale"]) and summary[1] == float(g["distance"])
        assert U.rel_err(np.array(odometry.overall_errors(got)), g["overall"]) <= U.RTOL
    else:
        assert summary[0] == 1.0


@pytest.mark.parametrize("align", [True, False])
def test_sequence_errors_thousand_poses_default_lengths(align):
    gt = odometry.trajectory_numpy(U.smooth_relative(999, seed=11, speed=0.75, dtype=np.float64))
    pred = odometry.trajectory_numpy(U.smooth_relative(999, seed=11, speed=0.75, bias=1.5e-3, scale=0.03))
    got, summary = _check_sequence(gt, pred, odometry.LENGTHS, odometry.STEP, align)
    assert 600 < summary[1] < 800 and 0 < len(got) < 100 * 8                  # 800 m never fits, 100 m often does
    assert 800.0 not in got[:, 3] and 100.0 in got[:, 3]


def test_sequence_errors_nothing_fits():
    gt = odometry.trajectory_numpy(U.smooth_relative(10, seed=2, dtype=np.float64))
    pred = odometry.trajectory_numpy(U.smooth_relative(10, seed=2, bias=1e-3, scale=0.03))
    got, summary = _check_sequence(gt, pred, odometry.LENGTHS, odometry.STEP, True)
    assert got.shape == (0, 5) and odometry.num_first_frames(11) == 2 and summary[1] > 5
    assert np.all(np.isnan(odometry.overall_errors(got)))


# ---- 5. the evaluator --------------------------------------------------------------------------------------------------------------

LENGTHS, STEP = (1.5, 3.0), 2


def _tree(tmp_path_factory):
    if "tree" not in _cache:
        from mono.datasets import KITTIOdomDataset, odom_sequence_files
        root = str(tmp_path_factory.mktemp("odom"))
        gt = U.make_sequence_tree(root, 9, 6)
        ds = KITTIOdomDataset(root, odom_sequence_files(9, 6), 32, 64, [0, 1], is_train=False, img_ext=".png")
        _cache["tree"] = (root, gt, ds)
    return _cache["tree"]


def _model():
    if "model" not in _cache:
        model = randomize_batchnorm(build_model("cfg_kitti_fm", 192, 640, seed=7))
        # A freshly initialised pose head gives |axis-angle|, |translation| < 1e-3: every rotation matrix is then the identity to
        # within one float32 ulp and a comparison of transforms measures the rounding of entries next to 1 (spacing 6e-8), not the
        # network.  x 64 (a power of two: the weights scale exactly) brings the pose vectors to the 0.01 ... 0.05 of a trained
        # network on KITTI, where 10 x the network's own cuda-vs-cpu distance (relative ~1e-6) is above that spacing.
        with torch.no_grad():
            model.PoseDecoder.conv3.weight.mul_(64.0)
            model.PoseDecoder.conv3.bias.mul_(64.0)
        _cache["model"] = model.to(_dev()).train()
    return _cache["model"]


def test_evaluator_metrics_are_the_host_statements(tmp_path_factory):
    _, gt, ds = _tree(tmp_path_factory)
    model = _model()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    res = odometry.OdometryEvaluator(model, _dev(), batch_size=4).evaluate(ds, gt, lengths=LENGTHS, step=STEP)      # 4 + 1 pairs
    assert model.training and all(m.training for m in model.modules()) and next(model.parameters()).is_cuda
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in state.items())
    assert res.relative.is_cuda and res.relative.shape == (5, 4, 4) and res.relative.dtype == torch.float32
    rel = res.relative.cpu().numpy()
    assert U.traj_err(res.poses, odometry.trajectory_numpy(rel)) <= U.RTOL
    assert U.rel_err(res.ates, odometry.snippet_ates_numpy(rel, gt)) <= U.RTOL
    rows, scale, distance = odometry.sequence_errors_numpy(gt, res.poses, LENGTHS, STEP)
    U.assert_conditions(rows, odometry.trajectory_distances(gt), LENGTHS, STEP)
    assert len(rows) >= 3 and res.segments.shape == rows.shape and np.array_equal(res.segments[:, [0, 3, 4]], rows[:, [0, 3, 4]])
    assert U.rel_err(res.segments[:, 1:3], rows[:, 1:3]) <= U.RTOL
    assert abs(res.scale - scale) <= U.RTOL * abs(scale) and res.distance == distance
    assert (res.t_err, res.r_err) == odometry.overall_errors(res.segments)
    assert res.ate_mean == float(np.mean(res.ates)) and res.ate_std == float(np.std(res.ates))


def test_evaluator_network_part_against_the_host(tmp_path_factory):
    """The relative transforms of the device path against the 'cpu' evaluator's, within 10 x the distance the parent's own
    PoseDecoder(PoseEncoder(x)) shows between cuda:0 and the CPU on the same pairs (max |difference| of its outputs, measured here;
    the margin covers Rodrigues' amplification at small angles).  Measured on one MI355X with the pose head as initialised
    (|output| <= 7.5e-4): network 4.2e-10, transforms 5.96e-8 = one float32 ulp of a diagonal entry next to 1, which no bound
    below the format's spacing can admit; hence the pose head of ``_model`` (see there)."""
    _, gt, ds = _tree(tmp_path_factory)
    model = _model().eval()
    try:
        host_model = build_model("cfg_kitti_fm", 192, 640, seed=7)
        host_model.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
        host_model.eval()
        pairs = odometry.pairs_torch(odometry.dataset_frames_u8(ds))
        with torch.no_grad():
            on_dev = model.PoseDecoder(model.PoseEncoder(pairs.to(_dev())))
            on_host = host_model.PoseDecoder(host_model.PoseEncoder(pairs))
        yardstick = max(float((a.cpu() - b).abs().max()) for a, b in zip(on_dev, on_host))
        dev_rel = odometry.OdometryEvaluator(model, _dev(), batch_size=4).relative_poses(ds).cpu()
        host_rel = odometry.OdometryEvaluator(host_model, "cpu", batch_size=4).relative_poses(ds)
        dist = float((dev_rel - host_rel).abs().max())
        print("network outputs cuda:0 vs cpu: %.3e; relative transforms: %.3e (bound %.3e); |output| max %.3e" % (
            yardstick, dist, 10 * yardstick, max(float(a.abs().max()) for a in on_host)))
        assert yardstick > 0 and dist <= 10 * yardstick
    finally:
        model.train()


def test_evaluator_bf16_and_foreign_model(tmp_path_factory):
    _, gt, ds = _tree(tmp_path_factory)
    model = _model()
    res = odometry.OdometryEvaluator(model, _dev(), batch_size=4, precision="bf16").evaluate(ds, gt, lengths=LENGTHS, step=STEP)
    assert model.training and np.all(np.isfinite(res.poses)) and np.all(np.isfinite(res.ates)) and np.all(np.isfinite(res.segments))
    assert np.isfinite(res.t_err) and np.isfinite(res.r_err) and np.isfinite(res.scale)
    # a model that lives on the host is copied, never moved
    host_model = build_model("cfg_kitti_fm", 192, 640, seed=7)
    rel = odometry.OdometryEvaluator(host_model, _dev(), batch_size=12).relative_poses(ds)
    assert rel.is_cuda and not next(host_model.parameters()).is_cuda


def test_eval_pose_script(tmp_path_factory, tmp_path):
    root, gt, ds = _tree(tmp_path_factory)
    ev = odometry.OdometryEvaluator(_model(), _dev(), batch_size=4)
    ckpt = str(tmp_path / "pose.pth")
    torch.save({"state_dict": {k: v.cpu() for k, v in _model().state_dict().items()}}, ckpt)
    out = str(tmp_path / "results")
    env = dict(os.environ, PYTHONPATH=U.ROOT)
    run = subprocess.run([sys.executable, os.path.join(U.ROOT, "scripts", "eval_pose.py"), "--config",
                          os.path.join(U.ROOT, "config", "cfg_kitti_fm.py"), "--checkpoint", ckpt, "--data_path", root, "--sequences", "9",
                          "--height", "32", "--width", "64", "--batch_size", "4", "--result_dir", out], env=env, capture_output=True,
                         text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    # The network is not bit-reproducible from one process to the next (MIOpen may pick another solver: 1e-10 on outputs of 1e-3
    # was seen), so the text is compared with the evaluator's scoring of the relative transforms the script itself recorded.
    child_rel = torch.from_numpy(np.load(os.path.join(out, "09_relative.npy"))).to(_dev())
    here_rel = ev.relative_poses(ds)
    print("relative transforms, child process vs this one: %.3e" % float((child_rel - here_rel).abs().max()))
    assert child_rel.shape == here_rel.shape and torch.allclose(child_rel, here_rel, rtol=0, atol=1e-5)      # the same checkpoint
    res = ev.evaluate(ds, gt, relative=child_rel)
    assert "odom_9 Trajectory error: {:0.3f}, std: {:0.3f}".format(res.ate_mean, res.ate_std) in run.stdout
    text = odometry.load_kitti_poses(os.path.join(out, "09_pred.txt"))
    assert text.shape == res.poses.shape
    assert np.all(np.abs(text - res.poses) <= 5.0000001e-9 * np.abs(res.poses) + 1e-300)           # %1.8e: 9 significant digits
    assert os.path.isfile(os.path.join(out, "09_eval", "09_error.txt")) and os.path.isfile(os.path.join(out, "09_eval", "09_stats.txt"))
