"""The host statement of PIL's LANCZOS resize (tripled_amd.resize) against PIL itself, bit for bit, and the 'raw_u8' wire format's
sample contract on a tiny KITTI-shaped tree.  No GPU."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import tripled_amd  # noqa: F401
from mmcv import ConfigDict
from mono.datasets.kitti_dataset import FLIP, LANCZOS, KITTIInpaintDataset, KITTIRAWDataset
from tripled_amd import resize

SHAPES = [((37, 53), (16, 24)),
          ((20, 30), (40, 64)),             # up-sampling: filter scale 1
          ((23, 64), (16, 64)),             # horizontal pass skipped
          ((16, 41), (16, 24)),             # vertical pass skipped
          ((9, 11), (7, 5)),                # support clipped at both edges
          ((375, 1242), (192, 640)),
          ((376, 1241), (320, 1024))]


def _image(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)      # binary: the worst overshoot into the clamp, both passes


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("kind", ["uniform", "binary"])
@pytest.mark.parametrize("src,dst", SHAPES)
def test_numpy_statement_is_bit_equal_to_pil(src, dst, kind, flip):
    img = _image(kind, src[0], src[1], seed=src[0] * 7 + dst[1])
    pil = Image.fromarray(img)
    if flip:
        pil = pil.transpose(FLIP)
    want = np.array(pil.resize((dst[1], dst[0]), LANCZOS))
    got = resize.lanczos_resize_numpy(img, dst[0], dst[1], flip=flip)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert int((got != want).sum()) == 0


@pytest.mark.parametrize("n_in,n_out", [(53, 24), (30, 64), (11, 5), (9, 7), (1242, 640), (376, 320)])
def test_coefficient_tables(n_in, n_out):
    k, bounds = resize.lanczos_coeffs(n_in, n_out)
    ksize = int(np.ceil(3.0 * max(n_in / n_out, 1.0))) * 2 + 1
    assert k.shape == (n_out, ksize) and k.dtype == np.int32
    assert bounds.shape == (n_out, 2) and bounds.dtype == np.int32
    sums = k.astype(np.int64).sum(1)
    assert int(np.abs(sums - (1 << 22)).max()) <= ksize            # every weight is rounded once
    assert int(bounds[:, 0].min()) >= 0 and int(bounds[:, 1].min()) >= 1
    assert int((bounds[:, 0] + bounds[:, 1]).max()) <= n_in and int(bounds[:, 1].max()) <= ksize
    for i in range(n_out):                                          # nothing beyond a row's count
        assert not k[i, bounds[i, 1]:].any()


def test_bank_layout_and_limits():
    bank = resize.LanczosBank([(37, 53), (16, 24)], 16, 24, "cpu")
    assert bank.canvas == (37, 53) and bank.desc.shape == (2, 8) and bank.tables.dtype == torch.int32
    h, w, ksx, ksy, okx, obx, oky, oby = (int(v) for v in bank.desc[0])
    kx, bx = resize.lanczos_coeffs(53, 24)
    ky, by = resize.lanczos_coeffs(37, 16)
    t = bank.host_tables
    assert (h, w, ksx, ksy) == (37, 53, kx.shape[1], ky.shape[1])
    assert np.array_equal(t[okx:okx + kx.size].reshape(ksx, 24), kx.T) and np.array_equal(t[obx:obx + 48].reshape(24, 2), bx)
    assert np.array_equal(t[oky:oky + ky.size].reshape(16, ksy), ky) and np.array_equal(t[oby:oby + 32].reshape(16, 2), by)
    # equal sizes: the pass PIL skips is the one-tap identity
    h, w, ksx, ksy, okx, obx, oky, oby = (int(v) for v in bank.desc[1])
    assert (ksx, ksy) == (1, 1) and set(t[okx:okx + 24]) == {1 << 22} and np.array_equal(t[obx:obx + 48:2], np.arange(24))
    with pytest.raises(ValueError):
        resize.LanczosBank([(8, 8)] * 17, 4, 4, "cpu")
    assert resize.get_bank([(37, 53)], 16, 24, "cpu") is resize.get_bank([(37, 53)], 16, 24, "cpu")


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """td_lanczos_resize_u8 validates on the host; nothing is launched (the device pointers are never dereferenced)."""
    import ctypes
    from tripled_amd import native
    lib = native.load()
    bank = resize.LanczosBank([(37, 53)], 16, 24, "cpu")
    desc = bank.desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    fake = ctypes.c_void_p(4096)
    n_ints = int(bank.tables.numel())

    def call(n_sizes=1, N=2, Hc=40, Wc=58, H=16, W=24, meta_host=None, src=fake, ints=n_ints, d=desc):
        return lib.td_lanczos_resize_u8(src, fake, meta_host, fake, ints, d, n_sizes, N, Hc, Wc, H, W, fake, fake, None)

    assert call(src=None) == -1 and call(N=0) == -1
    assert call(n_sizes=17) == -1 and call(n_sizes=0) == -1
    assert call(Hc=36) == -1 and call(Wc=52) == -1                          # a listed size larger than the canvas
    assert call(ints=n_ints - 1) == -1                                      # tables shorter than the description says
    assert call(meta_host=(ctypes.c_int * 4)(0, 0, 1, 0)) == -1             # a size index out of range
    assert call(meta_host=(ctypes.c_int * 4)(0, 1, -1, 0)) == -1
    assert call(src=ctypes.c_void_p(4097)) == -2                            # misaligned source
    wide = resize.LanczosBank([(8, 70000)], 8, 70000, "cpu")                # rows the LDS tile cannot hold
    assert lib.td_lanczos_resize_u8(fake, fake, None, fake, int(wide.tables.numel()), wide.desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                    1, 1, 8, 70000, 8, 70000, fake, fake, None) == -2


# ---- the wire format -----------------------------------------------------------------------------------------------------------

SIZES = [(40, 132), (37, 124)]
DRIVES = ["2011_09_26/2011_09_26_drive_0001_sync", "2011_09_26/2011_09_26_drive_0002_sync"]


def _make_tree(root, sizes=SIZES, n=3):
    files = []
    rng = np.random.RandomState(0)
    for drive, (h, w) in zip(DRIVES, sizes):
        for cam in ("image_02", "image_03"):
            d = os.path.join(root, drive, cam, "data")
            os.makedirs(d)
            for i in range(n):
                Image.fromarray(rng.randint(0, 255, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(d, "%010d.png" % i))
        files += ["%s %d l" % (drive, i) for i in range(n)]
    return files


def _seed(v):
    random.seed(v)
    torch.manual_seed(v)
    np.random.seed(v)


def test_raw_wire_sample_contract(tmp_path):
    files = _make_tree(str(tmp_path))
    H, W, frames = 16, 48, [0, -1, 1, "s"]
    common = dict(erase_shape=[4, 4], erase_count=3, raw_sizes=SIZES)
    raw_ds = KITTIInpaintDataset(str(tmp_path), files, H, W, frames, cfg=ConfigDict(wire="raw_u8", **common), is_train=True, img_ext=".png")
    u8_ds = KITTIInpaintDataset(str(tmp_path), files, H, W, frames, cfg=ConfigDict(wire="uint8", **common), is_train=True, img_ext=".png")
    flips = set()
    for seed in range(6):
        for index in (1, 4):                                       # one sample of each listed size
            _seed(seed)
            raw = raw_ds[index]
            _seed(seed)
            u8 = u8_ds[index]
            assert set(raw) == {("raw_u8", f) for f in frames} | {"raw_meta", "raw_spec", "aug", "K", "inv_K", "stereo_T", ("mask", 0, 0)}
            size_idx, flip = (int(v) for v in raw["raw_meta"])
            assert raw["raw_meta"].dtype == torch.int32 and raw["raw_meta"].shape == (2,)
            assert size_idx == (0 if index < 3 else 1) and flip in (0, 1)
            assert [int(v) for v in raw["raw_spec"]] == [H, W, 40, 132, 37, 124] and raw["raw_spec"].dtype == torch.int32
            flips.add(flip)
            for k in ("K", "inv_K", "stereo_T", "aug", ("mask", 0, 0)):      # the same draws in the same order
                assert torch.equal(raw[k], u8[k]), k
            assert raw[("mask", 0, 0)].shape == (3, H, W)
            h, w = SIZES[size_idx]
            for f in frames:
                canvas = raw[("raw_u8", f)]
                assert canvas.dtype == torch.uint8 and canvas.shape == (3, 40, 132)
                region = canvas[:, :h, :w].permute(1, 2, 0).numpy()
                got = resize.lanczos_resize_numpy(region, H, W, flip=bool(flip))
                assert np.array_equal(got, u8[("color_u8", f)].permute(1, 2, 0).numpy()), (seed, index, f)
    assert flips == {0, 1}


def test_raw_wire_refuses_an_unlisted_size(tmp_path):
    files = _make_tree(str(tmp_path))
    ds = KITTIRAWDataset(str(tmp_path), files, 16, 48, [0], cfg=ConfigDict(wire="raw_u8", raw_sizes=[(40, 132)]), is_train=False,
                         img_ext=".png")
    assert ds[0][("raw_u8", 0)].shape == (3, 40, 132)
    with pytest.raises(ValueError, match="raw_sizes"):
        ds[4]


def test_synthetic_raw_wire_matches_its_uint8_twin():
    from mono.datasets import SyntheticTripletDataset
    kw = dict(length=4, height=16, width=48, erase_shape=(4, 4), erase_count=2, augment=True, raw_sizes=SIZES)
    raw_ds, u8_ds = SyntheticTripletDataset(wire="raw_u8", **kw), SyntheticTripletDataset(wire="uint8", **kw)
    for i in range(4):
        raw, u8 = raw_ds[i], u8_ds[i]
        idx, flip = (int(v) for v in raw["raw_meta"])
        h, w = SIZES[idx]
        assert raw[("raw_u8", 0)].shape == (3, 40, 132) and torch.equal(raw["aug"], u8["aug"]) and torch.equal(raw["K"], u8["K"])
        for f in (0, -1, 1):
            region = raw[("raw_u8", f)][:, :h, :w].permute(1, 2, 0).numpy()
            assert np.array_equal(resize.lanczos_resize_numpy(region, 16, 48, flip=bool(flip)), u8[("color_u8", f)].permute(1, 2, 0).numpy())


def test_expansion_of_a_host_batch_is_refused():
    from mono.datasets import expand_device_batch
    from mono.datasets.raw_wire import raw_spec
    from tripled_amd import native
    batch = {("raw_u8", 0): torch.zeros(1, 3, 40, 132, dtype=torch.uint8), "raw_meta": torch.zeros(1, 2, dtype=torch.int32),
             "raw_spec": raw_spec(16, 48, SIZES).unsqueeze(0), "aug": torch.zeros(1, 9)}
    with pytest.raises(native.NativeLibraryError):
        expand_device_batch(batch)
    with pytest.raises(native.NativeLibraryError):
        resize.lanczos_resize_hip(batch[("raw_u8", 0)], batch["raw_meta"], resize.get_bank(SIZES, 16, 48, "cpu"))
