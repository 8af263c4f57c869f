"""csrc/td_surfel.hip on the device (tripled_amd.render.render_surfels_hip, tripled_amd.cloud_normals.orient_hip) against the numpy
statements, which tests/test_surfel_cpu.py pins to literal loops.  Every comparison is exact: np.array_equal on the float32 bits of
the depth and of the normal map, on the colours, the indices and the stats.  Both work distributions of the scatter kernel (one thread
per surfel; large boxes through the LDS queue) are held to the same statement.

Shapes: the smallest at which the kernels can go wrong.  One pixel and three points; 9 x 14 with 700 points and every planted point in
all eight modes; 3 x 300 (a row longer than a workgroup) at a radius where some boxes are drawn by their thread and some by a wave; 64
cameras of 5 x 7 with 20 011 points (32 blocks per camera: the grid-stride loop makes three passes, and the queue is drained in each);
a radius at which discs are capped; no points at all.  Orientation: one point and one camera, 700 x 3, and 20 011 points with 300
cameras (two LDS chunks)."""
import ctypes

import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tests import render_util as U
from tests import surfel_util as S
from tripled_amd import cloud_normals, native, render

pytestmark = pytest.mark.gpu

OWN = 4          # csrc/td_surfel.hip: TD_SURFEL_OWN


def _dev():
    return torch.device("cuda", 0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def run_hip(s, H, W, **kw):
    out = render.render_surfels_hip(_d(s.xyz), _d(s.rgb), _d(s.normals), _d(s.poses), s.K, H, W, **S.args(s, **kw))
    C = len(s.poses)
    assert [t.dtype for t in out] == [torch.float32, torch.uint8, torch.int32, torch.float32, torch.int64]
    assert [tuple(t.shape) for t in out] == [(C, H, W), (C, 3, H, W), (C, H, W), (C, 3, H, W), (C, 8)]
    return render.SurfelRendered(*(t.cpu().numpy() for t in out))


def check(s, H, W, **kw):
    """Both forms of the device against the statement -> the device's maps."""
    want = render.render_surfels_numpy(s.xyz, s.rgb, s.normals, s.poses, s.K, H, W, **S.args(s, **kw))
    for form in ("thread", "cooperative"):
        got = run_hip(s, H, W, form=form, **kw)
        S.assert_surfels_equal(got, want)
    return got


def clipped_areas(s, H, W, radius, camera=0):
    """Pixels of every drawn surfel's box inside the image, as the kernel clips it."""
    geo = render.surfel_setup_numpy(s.xyz, s.normals, s.poses[camera], s.K.reshape(-1), s.near, s.far, radius, 1.0, False, False, H, W)
    v = geo["visible"]
    x, y, r = geo["ui"][v], geo["vi"][v], geo["r"][v]
    return (np.minimum(W - 1, x + r) - np.maximum(0, x - r) + 1) * (np.minimum(H - 1, y + r) - np.maximum(0, y - r) + 1)


def test_the_smallest_case():
    got = check(S.scene(0, 3, 1, 1, 1), 1, 1)
    assert got.index[0, 0, 0] >= 0 and got.stats[0, 0] == 3


@pytest.mark.parametrize("mode", sorted(S.modes()))
def test_every_planted_surfel(mode):
    got = check(S.scene(0, 700, 3, 9, 14), 9, 14, **S.modes()[mode])
    st = dict(zip(render.SURFEL_STATS, got.stats.T))
    assert st["pixels_hit"].min() > 0 and st["billboards"][0] >= 1 and bool(st["culled"].any()) == S.modes()[mode]["cull"]


def test_a_row_longer_than_a_workgroup_with_boxes_of_both_kinds():
    s = S.scene(2, 1000, 2, 3, 300)
    areas = clipped_areas(s, 3, 300, 0.004)
    assert (areas <= OWN).sum() > 10 and (areas > OWN).sum() > 10            # drawn by their own thread, and by a wave from the queue
    got = check(s, 3, 300, radius=0.004)
    check(s, 3, 300, radius=0.1)                                             # and boxes wider than a wave
    assert got.stats[:, 7].min() > 0 and (got.index[:, :, 256:] >= 0).any()


def test_more_than_one_pass_of_the_grid_stride_loop():
    got = check(S.scene(3, 20011, 64, 5, 7), 5, 7, radius=0.2)
    assert (got.stats[:, 0] == 20011).all() and (got.index >= 32 * 256).any()      # a surfel of a later pass is on a picture
    # at 9 x 14 with larger discs: the queue is filled and drained in the later passes too, with boxes of more pixels than a wave has lanes
    s = S.scene(3, 20011, 64, 9, 14)
    geo = render.surfel_setup_numpy(s.xyz, s.normals, s.poses[0], s.K.reshape(-1), s.near, s.far, 0.15, 1.0, False, False, 9, 14)
    late = np.nonzero(geo["visible"])[0][clipped_areas(s, 9, 14, 0.15) > OWN]
    assert (late >= 32 * 256).any() and (late < 32 * 256).any()
    got = check(s, 9, 14, radius=0.15)
    assert (got.index >= 32 * 256).any()


def test_capped_discs():
    s = S.scene(0, 700, 3, 9, 14)
    got = check(s, 9, 14, radius=1.0)
    assert got.stats[:, 4].min() > 0
    p = s.planted["capped"]
    assert float(s.xyz[p, 2]) - 1.0 < s.near                                 # the disc reaches nearer than near


def test_no_points():
    got = check(S.scene(4, 0, 2, 33, 65), 33, 65, background=(7, 200, 31))
    assert not got.stats.any() and (got.index == -1).all() and not got.depth.any() and not got.normal.view(np.uint32).any()
    assert (got.color == np.array([7, 200, 31], np.uint8).reshape(1, 3, 1, 1)).all()


def test_two_runs_return_the_same_bits():
    s = S.scene(5, 1000, 2, 3, 300)
    workspace = render.render_workspace(4, 5, 300, _dev())                  # larger than needed, reused between the calls
    a = run_hip(s, 3, 300, radius=0.1, ambient=0.5, workspace=workspace)
    b = run_hip(s, 3, 300, radius=0.1, ambient=0.5, workspace=workspace)
    S.assert_surfels_equal(a, b)
    S.assert_surfels_equal(a, check(s, 3, 300, radius=0.1, ambient=0.5))


def test_a_short_workspace_is_refused_on_the_host():
    s = S.scene(0, 700, 3, 9, 14)
    short = torch.empty(3 * 9 * 14 - 1, dtype=torch.int64, device=_dev())    # one element short
    dev = [_d(a) for a in (s.xyz, s.rgb, s.normals, s.poses)]
    with pytest.raises(native.NativeLibraryError, match="workspace"):
        render.render_surfels_hip(*dev, s.K, 9, 14, 0.3, near=s.near, far=s.far, workspace=short)
    with pytest.raises(native.NativeLibraryError):                          # the workspace on the host
        render.render_surfels_hip(*dev, s.K, 9, 14, 0.3, near=s.near, far=s.far, workspace=short.cpu())
    # the C entry refuses it too, before anything is launched
    depth, color = torch.full((3, 9, 14), 77.0, device=_dev()), torch.empty(3, 3, 9, 14, dtype=torch.uint8, device=_dev())
    index, stats = torch.empty(3, 9, 14, dtype=torch.int32, device=_dev()), torch.full((3, 8), 77, dtype=torch.int64, device=_dev())
    nmap = torch.full((3, 3, 9, 14), 77.0, device=_dev())
    args = [dev[0], dev[1], dev[2], 700, dev[3], (ctypes.c_double * 9)(*s.K.reshape(-1)), 3, 9, 14, 1.0, s.near, s.far, 0.3, 0, 0, 1.0, 0,
            0, 0, 0, short, short.numel() * 8, depth, color, index, nmap, stats]
    with pytest.raises(native.NativeLibraryError):
        native.call("td_cloud_render_surfels", *args)
    torch.cuda.synchronize()
    assert bool((stats == 77).all()) and bool((depth == 77).all()) and bool((nmap == 77).all())


def check_orient(xyz, normals, poses, **kw):
    want = cloud_normals.orient_numpy(xyz, normals, poses, **kw)
    got = cloud_normals.orient_hip(_d(xyz), _d(normals), _d(poses), **kw)
    assert [t.dtype for t in got] == [torch.float32, torch.int32, torch.int64]
    got = [t.cpu().numpy() for t in got]
    assert np.array_equal(got[0].view(np.uint32), want.normal.view(np.uint32))
    assert np.array_equal(got[1], want.camera) and np.array_equal(got[2], want.stats)
    return want


def test_orientation():
    one = check_orient(np.array([[0.0, 0.0, 2.0]], np.float32), np.array([[0.0, 0.0, 1.0]], np.float32), np.eye(4)[None, :3].copy())
    assert one.stats.tolist() == [1, 0, 0, 0] and one.normal[0].tolist() == [0.0, 0.0, -1.0]
    s = S.scene(0, 700, 3, 9, 14)
    out = check_orient(s.xyz, s.normals, s.poses, pose_scale=1.5)
    assert (out.stats > 0).all()
    s = S.scene(3, 20011, 1, 5, 7)
    far = (6.0 * s.xyz).astype(np.float32)                                   # up to z = 120: beside cameras 256 ... 299 at z = 0.3 c
    out = check_orient(far, s.normals, U.trajectory(300))
    assert (out.camera >= cloud_normals.ORIENT_CHUNK).sum() > 100 and ((out.camera >= 0) & (out.camera < cloud_normals.ORIENT_CHUNK)).sum() > 100
    assert out.stats[0] > 1000 and out.stats[1] > 1000


def test_estimate_orients_on_the_device_as_on_the_host():
    g = np.random.default_rng(2)
    xy = g.uniform(-1.0, 1.0, (900, 2))
    xyz = np.stack([xy[:, 0], xy[:, 1], 0.05 * np.sin(3.0 * xy[:, 0]) + 0.001 * g.normal(size=900) + 2.0], 1)
    poses = U.trajectory(3)
    host = cloud_normals.CloudNormals("cpu", 0.5, min_neighbours=6, max_curvature=0.05).estimate(xyz, poses=poses, pose_scale=0.5)
    dev = cloud_normals.CloudNormals(_dev(), 0.5, min_neighbours=6, max_curvature=0.05).estimate(xyz, poses=poses, pose_scale=0.5)
    assert dev.normal.is_cuda and dev.normal.dtype == torch.float64
    assert np.array_equal(dev.normal.cpu().numpy().view(np.uint64), host.normal.view(np.uint64))
    assert dev.stats == host.stats and host.stats["orient_flipped"] > 100 and host.stats["valid"] > 300


def test_renderer_batches_surfels():
    """One render_surfels() call with more cameras than batch_size equals the host path."""
    s = S.scene(6, 700, 7, 9, 14)
    params = dict(near=s.near, far=s.far)
    kw = dict(radius=S.RADIUS, cull=True, ambient=0.25)
    want = render.CloudRenderer("cpu", 9, 14, s.K, **params).render_surfels(s.xyz, s.rgb, s.normals, s.poses, **kw)
    renderer = render.CloudRenderer("cuda", 9, 14, s.K, batch_size=3, **params)
    got = renderer.render_surfels(s.xyz, s.rgb, s.normals, s.poses, **kw)    # 3 + 3 + 1 cameras
    assert all(isinstance(a, np.ndarray) for a in got) and renderer._workspace.numel() == 3 * 9 * 14 * 8
    S.assert_surfels_equal(got, want)
    resident = renderer.upload(s.xyz, s.rgb)
    S.assert_surfels_equal(renderer.render_surfels(*resident, _d(s.normals), s.poses[2:6], **kw), render.SurfelRendered(*(a[2:6] for a in want)))
    pose, K = render.top_view(s.xyz, 9, 14, near=s.near)                    # a top view through the orthographic branch
    far = 3 * s.near + float(np.nanmax(s.xyz[:, 1]) - np.nanmin(s.xyz[:, 1]))
    top = renderer.render_surfels(*resident, s.normals, pose[None], K=K, ortho=True, far=far, radius=S.RADIUS)
    S.assert_surfels_equal(top, render.render_surfels_numpy(s.xyz, s.rgb, s.normals, pose[None], K, 9, 14, S.RADIUS, ortho=True,
                                                            **dict(params, far=far)))
