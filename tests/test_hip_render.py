"""csrc/td_render.hip on the device (through tripled_amd.render.render_hip) against the numpy statement, which
tests/test_render_cpu.py pins to a literal per-pixel loop.  Every comparison is exact: np.array_equal on the float32 bits of the depth,
on the colours, the indices and the stats.  Every table entry of the kernel is a minimum of integers and the projection a fixed
sequence of individually rounded float64 operations.

Shapes: the smallest at which the kernels can go wrong.  One pixel and three points; 9 x 14 with 700 points and every planted point
(rows shorter than a wave) in all four modes; 3 x 300 (a row longer than a workgroup); 64 cameras of 5 x 7 with 20 011 points (the
per-camera block count sits at its lower clamp of 32, 32 x 256 = 8192 threads: the grid-stride loop makes three passes); no points
at all.  An index beyond 2^31 is not run: the entry point refuses such a cloud, and a plane of 2^31 pixels as well."""
import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tests import render_util as U
from tripled_amd import native, render

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def run_hip(s, H, W, **kw):
    out = render.render_hip(_d(s.xyz), _d(s.rgb), _d(s.poses), s.K, H, W, **U.render_args(s, **kw))
    C = len(s.poses)
    assert [t.dtype for t in out] == [torch.float32, torch.uint8, torch.int32, torch.int64]
    assert [tuple(t.shape) for t in out] == [(C, H, W), (C, 3, H, W), (C, H, W), (C, 5)]
    return render.Rendered(*(t.cpu().numpy() for t in out))


def check(s, H, W, **kw):
    """The device against the statement -> the device's maps."""
    got = run_hip(s, H, W, **kw)
    want = render.render_numpy(s.xyz, s.rgb, s.poses, s.K, H, W, **U.render_args(s, **{k: v for k, v in kw.items() if k != "workspace"}))
    U.assert_rendered_equal(got, want)
    return got


def test_the_smallest_case():
    got = check(U.scene(0, 3, 1, 1, 1), 1, 1)
    assert got.index[0, 0, 0] == 0 and got.stats[0, 0] == 3


@pytest.mark.parametrize("mode", ["none", "mixed", "saturated", "ortho"])
def test_every_special_point(mode):
    got = check(U.scene(0, 700, 3, 9, 14), 9, 14, **U.modes(14)[mode])
    assert (got.stats.sum(0) > 0).all()


def test_a_row_longer_than_a_workgroup():
    got = check(U.scene(2, 1000, 2, 3, 300), 3, 300, splat=U.mixed_splat(300))
    assert got.stats[:, 4].min() > 0 and (got.index[:, :, 256:] >= 0).any()


def test_more_than_one_pass_of_the_grid_stride_loop():
    got = check(U.scene(3, 20011, 64, 5, 7), 5, 7)
    assert (got.stats[:, 0] == 20011).all() and (got.index >= 32 * 256).any()      # a point of a later pass is on a picture


def test_no_points():
    got = check(U.scene(4, 0, 2, 33, 65), 33, 65, background=(7, 200, 31))
    assert not got.stats.any() and (got.index == -1).all() and not got.depth.any()
    assert (got.color == np.array([7, 200, 31], np.uint8).reshape(1, 3, 1, 1)).all()


def test_background_and_pose_scale():
    s = U.scene(0, 700, 3, 9, 14)
    got = check(s, 9, 14, background=(255, 1, 128), pose_scale=0.5)
    assert (got.color.transpose(0, 2, 3, 1)[got.index < 0] == np.array([255, 1, 128], np.uint8)).all() and (got.index < 0).any()
    other = check(s, 9, 14, splat=U.mixed_splat(14), pose_scale=1.75)
    assert not np.array_equal(other.index[1:], got.index[1:])


def test_two_runs_return_the_same_bits():
    s = U.scene(5, 1000, 2, 3, 300)
    workspace = render.render_workspace(4, 5, 300, _dev())                  # larger than needed, reused between the calls
    a = run_hip(s, 3, 300, splat=U.saturating_splat(300), workspace=workspace)
    b = run_hip(s, 3, 300, splat=U.saturating_splat(300), workspace=workspace)
    U.assert_rendered_equal(a, b)
    U.assert_rendered_equal(a, check(s, 3, 300, splat=U.saturating_splat(300)))


def test_a_short_workspace_is_refused_on_the_host():
    s = U.scene(0, 700, 3, 9, 14)
    short = torch.empty(3 * 9 * 14 - 1, dtype=torch.int64, device=_dev())    # one element short
    with pytest.raises(native.NativeLibraryError, match="workspace"):
        render.render_hip(_d(s.xyz), _d(s.rgb), _d(s.poses), s.K, 9, 14, near=s.near, far=s.far, workspace=short)
    with pytest.raises(native.NativeLibraryError):                          # the workspace on the host
        render.render_hip(_d(s.xyz), _d(s.rgb), _d(s.poses), s.K, 9, 14, near=s.near, far=s.far, workspace=short.cpu())
    # the C entry refuses it too, before anything is launched
    xyz, rgb, poses = _d(s.xyz), _d(s.rgb), _d(s.poses)
    depth, color = torch.full((3, 9, 14), 77.0, device=_dev()), torch.empty(3, 3, 9, 14, dtype=torch.uint8, device=_dev())
    index, stats = torch.empty(3, 9, 14, dtype=torch.int32, device=_dev()), torch.full((3, 5), 77, dtype=torch.int64, device=_dev())
    import ctypes
    args = [xyz, rgb, 700, poses, (ctypes.c_double * 9)(*s.K.reshape(-1)), 3, 9, 14, 1.0, s.near, s.far, 0.0, 0, 0, 0, 0, short,
            short.numel() * 8, depth, color, index, stats]
    with pytest.raises(native.NativeLibraryError):
        native.call("td_cloud_render", *args)
    torch.cuda.synchronize()
    assert bool((stats == 77).all()) and bool((depth == 77).all())


def test_renderer_batches():
    """One render() call with more cameras than batch_size equals the single-batch result (and the statement)."""
    s = U.scene(6, 700, 7, 9, 14)
    params = dict(near=s.near, far=s.far, splat=U.mixed_splat(14))
    whole = render.CloudRenderer(_dev(), 9, 14, s.K, batch_size=12, **params).render(s.xyz, s.rgb, s.poses)
    renderer = render.CloudRenderer("cuda", 9, 14, s.K, batch_size=3, **params)
    parts = renderer.render(s.xyz, s.rgb, s.poses)                          # 3 + 3 + 1 cameras
    assert all(isinstance(a, np.ndarray) for a in parts) and renderer._workspace.numel() == 3 * 9 * 14 * 8
    U.assert_rendered_equal(parts, whole)
    U.assert_rendered_equal(parts, render.render_numpy(s.xyz, s.rgb, s.poses, s.K, 9, 14, **params))
    resident = renderer.upload(s.xyz, s.rgb)                                # the cloud stays on the device between calls
    assert resident[0].is_cuda
    U.assert_rendered_equal(renderer.render(*resident, s.poses[2:6]), render.Rendered(*(a[2:6] for a in whole)))
    pose, K = render.top_view(s.xyz, 9, 14, near=s.near)                    # and a top view through the same renderer
    far = 3 * s.near + float(np.nanmax(s.xyz[:, 1]) - np.nanmin(s.xyz[:, 1]))
    top = renderer.render(*resident, pose[None], K=K, ortho=True, far=far)
    U.assert_rendered_equal(top, render.render_numpy(s.xyz, s.rgb, pose[None], K, 9, 14, ortho=True, **dict(params, far=far)))
    assert top.stats[0, 3] == 699                                           # everything but the NaN is inside the box
