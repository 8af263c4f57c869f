"""The 'resident' wire format without a GPU (tripled_amd.resident, tools/pack_frames.py): the packer and the store format, the sample
contract next to the 'raw_u8' wire's, the host statement of the indexed resize, the errors, and the entry point's argument checks."""
import atexit
import ctypes
import functools
import json
import os
import random
import shutil
import tempfile

import numpy as np
import pytest
import torch
from PIL import Image

import tripled_amd  # noqa: F401
from mmcv import ConfigDict
from mono.datasets.kitti_dataset import KITTIInpaintDataset
from tripled_amd import native, resident, resize

SIZES = [(20, 30), (23, 31)]
H, W = 16, 24
DRIVES = {".png": ("2011_09_26/2011_09_26_drive_0001_sync", SIZES[0]), ".jpg": ("2011_09_28/2011_09_28_drive_0002_sync", SIZES[1])}
N_FRAMES = 5
FRAME_IDS = [0, -1, 1, "s"]


def make_tree(root):
    """Two drives of 5 frames, both sides: one of 20x30 .png files, one of 23x31 .jpg files."""
    rng = np.random.RandomState(0)
    for ext, (drive, (h, w)) in DRIVES.items():
        for cam in ("image_02", "image_03"):
            d = os.path.join(root, drive, cam, "data")
            os.makedirs(d)
            for i in range(N_FRAMES):
                Image.fromarray(rng.randint(0, 255, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(d, "%010d%s" % (i, ext)))


def files_of(ext):
    return ["%s %d %s" % (DRIVES[ext][0], i, "lr"[i % 2]) for i in range(N_FRAMES)]


def dataset(root, ext, wire, store=None, frame_ids=FRAME_IDS, cls=KITTIInpaintDataset, files=None, raw_sizes=SIZES, train=True):
    cfg = ConfigDict(wire=wire, store=store, raw_sizes=raw_sizes, erase_shape=[4, 4], erase_count=3)
    return cls(root, files_of(ext) if files is None else files, H, W, list(frame_ids), cfg=cfg, is_train=train, img_ext=ext)


@functools.lru_cache(maxsize=None)
def packed_tree():
    """(tree root, {ext: store directory}) -- written and packed once, shared by the tests, never changed."""
    root = tempfile.mkdtemp(prefix="td_resident_")
    atexit.register(shutil.rmtree, root, ignore_errors=True)
    tree = os.path.join(root, "kitti")
    make_tree(tree)
    stores = {}
    for ext in DRIVES:
        stores[ext] = os.path.join(root, "store_" + ext[1:])
        resident.pack([dataset(tree, ext, "raw_u8")], stores[ext], workers=0)
    return tree, stores


def _planar(path):
    return np.ascontiguousarray(np.array(Image.open(path).convert("RGB")).transpose(2, 0, 1))


def _seed(v):
    random.seed(v)
    torch.manual_seed(v)
    np.random.seed(v)


# ---- the packer -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ext", [".png", ".jpg"])
def test_pack_holds_every_frame_once_aligned(ext):
    tree, stores = packed_tree()
    doc = json.load(open(os.path.join(stores[ext], "store.json")))
    blob = np.fromfile(os.path.join(stores[ext], "store.bin"), dtype=np.uint8)
    drive, (h, w) = DRIVES[ext]
    want = sorted("%s/%s/data/%010d%s" % (drive, cam, i, ext) for cam in ("image_02", "image_03") for i in range(N_FRAMES))
    paths = [e[0] for e in doc["frames"]]
    assert paths == want                                        # both sides (the 's' frame id) and every neighbour, each once
    assert doc["version"] == 1 and doc["ext"] == ext and doc["raw_sizes"] == [[h, w]] and doc["total_bytes"] == blob.size
    end = 0
    for path, fh, fw, off in doc["frames"]:
        assert (fh, fw) == (h, w) and off % 16 == 0 and off >= end
        assert not blob[end:off].any()                          # the padding
        frame = _planar(os.path.join(tree, path))
        assert np.array_equal(blob[off:off + frame.size].reshape(frame.shape), frame), path
        end = off + frame.size
    assert end == blob.size


def test_packing_twice_gives_identical_files(tmp_path):
    """The second time through decoder processes: the order of the frames does not depend on who decodes them."""
    tree, stores = packed_tree()
    again = str(tmp_path / "again")
    info = resident.pack([dataset(tree, ".png", "raw_u8")], again, workers=2)
    assert info["frames"] == 2 * N_FRAMES and info["bytes"] == os.path.getsize(os.path.join(again, "store.bin"))
    for name in ("store.bin", "store.json"):
        assert open(os.path.join(again, name), "rb").read() == open(os.path.join(stores[".png"], name), "rb").read(), name
    assert sorted(os.listdir(again)) == ["store.bin", "store.json"]          # no pickles, nothing else


def test_pack_lists_neighbours_only_where_they_exist(tmp_path):
    tree, _ = packed_tree()
    ds = dataset(tree, ".png", "raw_u8", frame_ids=[0, -1, 1], files=["%s 0 l" % DRIVES[".png"][0], "%s 4 l" % DRIVES[".png"][0]])
    resident.pack([ds], str(tmp_path), workers=0)
    names = [e[0].rsplit("/", 1)[1] for e in json.load(open(str(tmp_path / "store.json")))["frames"]]
    assert names == ["%010d.png" % i for i in (0, 1, 3, 4)]                   # -1 and 5 do not exist: simply absent


def test_pack_refuses_an_unlisted_size(tmp_path):
    tree, _ = packed_tree()
    with pytest.raises(ValueError, match="raw_sizes"):
        resident.pack([dataset(tree, ".jpg", "raw_u8", raw_sizes=[SIZES[0]])], str(tmp_path), workers=0)
    assert not os.path.exists(str(tmp_path / "store.bin"))


# ---- the sample contract --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ext", [".png", ".jpg"])
def test_resident_samples_take_the_draws_of_the_raw_wire(ext):
    """Interior, first and last frame of a drive (neighbour fallback), frame_ids [0, -1, 1, 's'], in-painting masks: everything but
    the frames themselves is equal, the bytes at each offset are the canvas's valid region, and both paths leave the generators in
    the same state."""
    tree, stores = packed_tree()
    res_ds, raw_ds = dataset(tree, ext, "resident", stores[ext]), dataset(tree, ext, "raw_u8")
    blob = np.fromfile(os.path.join(stores[ext], "store.bin"), dtype=np.uint8)
    size_idx = SIZES.index(DRIVES[ext][1])
    h, w = SIZES[size_idx]
    flips, jitters = set(), set()
    for seed in range(5):
        for index in (2, 0, N_FRAMES - 1):
            _seed(seed)
            raw = raw_ds[index]
            raw_state = (random.getstate(), torch.get_rng_state())
            _seed(seed)
            opened = []
            res_ds.loader = lambda path: opened.append(path)                # the resident wire opens no image file
            res = res_ds[index]
            assert not opened
            assert random.getstate() == raw_state[0] and torch.equal(torch.get_rng_state(), raw_state[1])
            assert set(res) == {("res_off", f) for f in FRAME_IDS} | {"raw_meta", "raw_spec", "res_bytes", "aug", "K", "inv_K", "stereo_T",
                                                                      ("mask", 0, 0)}
            for k in ("raw_meta", "raw_spec", "aug", "K", "inv_K", "stereo_T", ("mask", 0, 0)):
                assert torch.equal(res[k], raw[k]) and res[k].dtype == raw[k].dtype, k
            assert int(res["raw_meta"][0]) == size_idx and int(res["res_bytes"]) == blob.size and res["res_bytes"].dtype == torch.int64
            flips.add(int(res["raw_meta"][1]))
            jitters.add(float(res["aug"][0]))
            for f in FRAME_IDS:
                off = res[("res_off", f)]
                assert off.dtype == torch.int64 and off.dim() == 0
                got = blob[int(off):int(off) + 3 * h * w].reshape(3, h, w)
                assert np.array_equal(got, raw[("raw_u8", f)][:, :h, :w].numpy()), (seed, index, f)
            if index == 0:
                assert int(res[("res_off", -1)]) == int(res[("res_off", 0)])          # no frame -1: the centre frame
            if index == N_FRAMES - 1:
                assert int(res[("res_off", 1)]) == int(res[("res_off", 0)])
            assert int(res[("res_off", "s")]) != int(res[("res_off", 0)])
    assert flips == {0, 1} and jitters == {0.0, 1.0}


@pytest.mark.parametrize("flip", [0, 1])
def test_host_statement_equals_the_resize_of_the_decoded_file(flip):
    tree, stores = packed_tree()
    for ext in DRIVES:
        index = resident.load_index(stores[ext])
        blob = np.memmap(os.path.join(stores[ext], "store.bin"), dtype=np.uint8, mode="r")
        paths = sorted(index.frames)[::3]
        offsets = [index.frames[p][0] for p in paths]
        size_idx = SIZES.index(DRIVES[ext][1])
        got = resident.resize_from_store_numpy(blob, offsets, [(size_idx, flip)] * len(paths), SIZES, H, W)
        assert got.shape == (len(paths), 3, H, W) and got.dtype == np.uint8
        for g, p in zip(got, paths):
            img = np.array(Image.open(os.path.join(tree, p)).convert("RGB"))
            assert np.array_equal(g, resize.lanczos_resize_numpy(img, H, W, flip=bool(flip)).transpose(2, 0, 1)), p
    with pytest.raises(ValueError, match="leaves the store"):
        resident.resize_from_store_numpy(blob, [blob.size - 10], [(0, 0)], SIZES, H, W)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------

def test_a_centre_frame_absent_from_the_index_raises(tmp_path):
    tree, _ = packed_tree()
    drive = DRIVES[".png"][0]
    resident.pack([dataset(tree, ".png", "raw_u8", frame_ids=[0], files=["%s 1 l" % drive])], str(tmp_path), workers=0)
    ds = dataset(tree, ".png", "resident", str(tmp_path), frame_ids=[0, -1, 1], files=["%s 1 l" % drive, "%s 3 l" % drive])
    sample = ds[0]                                              # neighbours the packer was not asked for: the centre frame
    assert int(sample[("res_off", -1)]) == int(sample[("res_off", 0)]) == int(sample[("res_off", 1)])
    with pytest.raises(ValueError, match=r"store\.json does not list .*0000000003\.png"):
        ds[1]


def test_an_index_that_disagrees_with_the_config_raises():
    tree, stores = packed_tree()
    with pytest.raises(ValueError, match=r"store\.json was packed from '\.png' images"):
        dataset(tree, ".jpg", "resident", stores[".png"])[0]
    with pytest.raises(ValueError, match=r"store\.json holds frames of the sizes \[\(23, 31\)\]"):
        dataset(tree, ".jpg", "resident", stores[".jpg"], raw_sizes=[SIZES[0]])[0]
    with pytest.raises(ValueError, match="cfg.data.store"):
        dataset(tree, ".png", "resident", None)[0]


def test_frames_of_one_sample_with_different_sizes_raise(tmp_path):
    tree, stores = packed_tree()
    doc = json.load(open(os.path.join(stores[".png"], "store.json")))
    doc["frames"][1][1:3] = [23, 31]                             # frame 1 of image_02 claims the other listed size
    doc["raw_sizes"] = [list(s) for s in SIZES]
    os.makedirs(str(tmp_path / "s"))
    json.dump(doc, open(str(tmp_path / "s" / "store.json"), "w"))
    ds = dataset(tree, ".png", "resident", str(tmp_path / "s"), frame_ids=[0, 1], files=["%s 0 l" % DRIVES[".png"][0]])
    with pytest.raises(ValueError, match=r"different sizes in .*store\.json"):
        ds[0]


def test_a_store_needs_a_device():
    _, stores = packed_tree()
    with pytest.raises(native.NativeLibraryError, match="device memory"):
        resident.ResidentStore(stores[".png"], "cpu")
    with pytest.raises(native.NativeLibraryError, match="device memory"):
        resident.resize_from_store_hip(torch.zeros(4096, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64),
                                       torch.zeros(1, 2, dtype=torch.int32), resize.get_bank(SIZES, H, W, "cpu"))


def test_expansion_of_a_host_batch_is_refused():
    from mono.datasets import expand_device_batch
    tree, stores = packed_tree()
    sample = dataset(tree, ".png", "resident", stores[".png"])[1]
    with pytest.raises(native.NativeLibraryError, match="resident wire format"):
        expand_device_batch({k: v.unsqueeze(0) for k, v in sample.items()})


def test_offsets_keep_their_bits_through_staging_rules():
    from mono.datasets.raw_wire import HOST_KEYS, keeps_dtype
    assert keeps_dtype(("res_off", -1)) and keeps_dtype(("res_off", "s")) and keeps_dtype("raw_meta") and keeps_dtype(("raw_u8", 0))
    assert not keeps_dtype("K") and not keeps_dtype(("color", 0, 0)) and "res_bytes" in HOST_KEYS and "raw_spec" in HOST_KEYS


# ---- the entry point ------------------------------------------------------------------------------------------------------------------

def test_entry_point_refuses_bad_arguments_before_any_launch():
    """td_lanczos_resize_u8_indexed validates on the host; nothing is launched (the device pointers are never dereferenced)."""
    lib = native.load()
    assert lib.td_abi_version() == 3
    bank = resize.LanczosBank(SIZES, H, W, "cpu")
    desc = bank.desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    fake = ctypes.c_void_p(4096)
    n_ints = int(bank.tables.numel())
    store_bytes = 10000
    ll = lambda *v: (ctypes.c_longlong * len(v))(*v)        # noqa: E731
    ints = lambda *v: (ctypes.c_int * len(v))(*v)           # noqa: E731

    def call(store=fake, nbytes=store_bytes, offsets=fake, off_host=None, meta=fake, meta_host=None, tables=fake, n=n_ints, d=desc,
             n_sizes=2, N=2, dst=fake, status=fake):
        return lib.td_lanczos_resize_u8_indexed(store, nbytes, offsets, off_host, meta, meta_host, tables, n, d, n_sizes, N, H, W, dst,
                                                status, None)

    for null in ("store", "offsets", "meta", "tables", "d", "dst", "status"):
        assert call(**{null: None}) == -1, null
    assert call(N=0) == -1 and call(N=-3) == -1 and call(nbytes=0) == -1
    assert call(n_sizes=0) == -1 and call(n_sizes=17) == -1 and call(n=n_ints - 1) == -1
    assert call(meta_host=ints(0, 0, 2, 0)) == -1                                       # a size index out of range
    f0, f1 = 3 * 20 * 30, 3 * 23 * 31
    # host offsets outside the store: negative, past the end, a frame that straddles the end -- by the frame's own size with meta_host
    assert call(off_host=ll(0, -1)) == -1 and call(off_host=ll(store_bytes, 0)) == -1
    assert call(off_host=ll(0, store_bytes - f1 + 1), meta_host=ints(0, 0, 1, 1)) == -1
    assert call(off_host=ll(0, store_bytes - f0 + 1)) == -1                             # without meta_host: the smallest frame
    assert call(nbytes=f0 - 1, off_host=ll(0, 0)) == -1                                 # a store smaller than one frame
    # in range: the arguments pass the checks, and a misaligned store is 'unsupported', still before any launch
    assert call(store=ctypes.c_void_p(4097), off_host=ll(0, store_bytes - f1), meta_host=ints(0, 0, 1, 1)) == -2
    assert call(store=ctypes.c_void_p(4097), off_host=ll(3, store_bytes - f0)) == -2
    assert b"bad argument" in lib.td_error_string(-1)
