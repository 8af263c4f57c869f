"""tripled_amd.infer's host statements against the REAL reference programs: scripts/infer.py (transform, predict) and
scripts/eval_depth_pp.py (batch_post_process_disparity), loaded stand-alone from /root/reference with their cv2 / mmcv / mono
imports stubbed and Tensor.cuda() a no-op (tools/gen_golden_infer.load_reference; everything is patched through monkeypatch and
undone after each test).  Skipped where the reference checkout is absent (the GPU box): tests/golden/infer.npz carries the
same comparisons there (test_infer_cpu.py, test_hip_infer.py)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import infer
from tests.infer_util import ROOT, golden, smooth_disp, smooth_image

REF_ROOT = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF_ROOT, "scripts", "infer.py")),
                                reason="reference checkout not present")


@pytest.fixture
def ref(monkeypatch):
    spec = importlib.util.spec_from_file_location("_gen_golden_infer", os.path.join(ROOT, "tools", "gen_golden_infer.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ref_infer, ref_pp = gen.load_reference(REF_ROOT, monkeypatch)
    return gen, ref_infer, ref_pp


@pytest.mark.parametrize("shape", [(37, 53, 32, 64), (75, 248, 96, 320), (64, 100, 96, 320), (120, 400, 320, 1024)])
def test_preprocess_is_the_references_transform(ref, shape):
    _, ref_infer, _ = ref
    H0, W0, h, w = shape
    img = smooth_image(H0 + w, H0, W0)
    want = ref_infer.transform(img, h, w)
    got = infer.preprocess_torch(img, h, w)
    assert got.dtype == want.dtype and torch.equal(got, want)          # the same torch call: bit for bit


@pytest.mark.parametrize("B,h,w,H0,W0", [(1, 32, 64, 37, 53), (2, 48, 160, 94, 311), (3, 96, 320, 64, 100)])
def test_postprocess_paired_is_the_references_blend_then_resize(ref, B, h, w, H0, W0):
    _, _, ref_pp = ref
    net = smooth_disp(B * 7 + h, 2 * B, h, w)
    l, r = net[:B, 0].numpy(), net[B:, 0].numpy()[:, :, ::-1]
    blended = ref_pp.batch_post_process_disparity(l, r)               # float64
    want = torch.nn.functional.interpolate(torch.from_numpy(blended.astype(np.float32))[:, None], (H0, W0), mode="bilinear",
                                           align_corners=False)[:, 0]
    got, _ = infer.postprocess_torch(net, H0, W0, paired=True)
    err = float((got - want).abs().max())
    print("paired disparity vs reference (B %d, %dx%d -> %dx%d): max abs %.3e" % (B, h, w, H0, W0, err))
    assert err <= 1e-6


@pytest.mark.parametrize("size", [(24, 40), (93, 307)])
def test_predict_matches_the_references_predict(ref, size):
    """Stub model = mean over the channels; the reference hard-codes the 320 x 1024 network size."""
    gen, ref_infer, _ = ref
    img = smooth_image(size[0], *size)
    want_depth, want_disp = ref_infer.predict(img, gen.channel_mean_model)

    class Mean(torch.nn.Module):
        def forward(self, inputs):
            return gen.channel_mean_model(inputs)

    p = infer.DepthPredictor(Mean(), 320, 1024, "cpu", affine=infer.REFERENCE_AFFINE, depth_scale=infer.REFERENCE_DEPTH_SCALE)
    pred = p.predict([img])
    np.testing.assert_allclose(pred.disp[0].numpy(), want_disp, rtol=0, atol=1e-6)
    np.testing.assert_allclose(pred.depth[0].numpy(), want_depth, rtol=1e-5, atol=0)


def test_fixture_is_what_the_generator_records(ref):
    """tests/golden/infer.npz is reproducible from the reference as it stands (everything but the picture bytes, which
    need matplotlib: those are covered by test_infer_cpu.test_committed_table_is_matplotlibs_magma)."""
    gen, ref_infer, ref_pp = ref
    pytest.importorskip("matplotlib")
    fresh, stored = gen.record(ref_infer, ref_pp), golden()
    assert sorted(fresh) == sorted(stored.files)
    for k in stored.files:
        assert np.array_equal(fresh[k], stored[k]), k
