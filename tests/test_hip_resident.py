"""The 'resident' wire format on the device: td_lanczos_resize_u8_indexed (csrc/td_resize.hip) against its host statement, bit for bit
(torch.equal everywhere: there is no tolerance in this feature), the guards of the store's edges, and the wire end to end --
expansion, staging, graph capture, train_mono -- next to the 'raw_u8' wire on the same fabricated tree.

The references of the resize are those of tests/test_hip_resize.py (its cached ``_case``), so each is computed once for both files."""
import functools
import json
import os
import random

import numpy as np
import pytest
import torch

from tests.test_hip_resize import KITTI, _canvases, _case
from tests.test_resident_cpu import dataset, packed_tree

pytestmark = pytest.mark.gpu

RESERVE_GB = 1.0          # the tests' stores are a few KB; the default reserve (32 GB) is the product's, for a training run


def _dev():
    return torch.device("cuda", 0)


def _four(k):
    """Shape pair k of the small set as FOUR images -- uniform, binary flipped, binary, uniform flipped -- with their references."""
    a, b = _case(str(k)), _case("%db" % k)
    return a[0] + b[0], a[2] + b[2], a[3], a[5], torch.cat([a[6], b[6]])


def _planar(region):
    return np.ascontiguousarray(region.transpose(2, 0, 1)).reshape(-1)


def _place(regions, residues, seed, lead=0, tail_mod=None):
    """A store of random bytes with the frames at offsets of the given residues mod 4 (``lead`` = 0: the first frame at offset 0),
    odd gaps in between; ``tail_mod``: the last frame ends on the store's last byte and the length is tail_mod mod 4."""
    rng = np.random.default_rng(seed)
    offsets, pos = [], lead
    for region, res in zip(regions, residues):
        while pos % 4 != res:
            pos += 1
        offsets.append(pos)
        pos += region.size + 5
    if tail_mod is None:
        total = pos + 7
    else:
        total = offsets[-1] + regions[-1].size
        while total % 4 != tail_mod:                            # move the last frame so that the store ends with it
            total += 1
        offsets[-1] = total - regions[-1].size
        assert offsets[-1] >= offsets[-2] + regions[-2].size if len(offsets) > 1 else True
    store = rng.integers(0, 256, total, dtype=np.uint8)
    for region, off in zip(regions, offsets):
        store[off:off + region.size] = _planar(region)
    return store, offsets


def _run(store, offsets, idx, flips, sizes, out, device_args=True):
    import tripled_amd  # noqa: F401
    from tripled_amd import resident, resize
    dev = _dev()
    bank = resize.get_bank(sizes, out[0], out[1], dev)
    meta = torch.tensor(list(zip(idx, flips)), dtype=torch.int32)
    off = torch.tensor(offsets, dtype=torch.int64)
    if device_args:
        meta, off = meta.to(dev), off.to(dev)
    data = store if torch.is_tensor(store) else torch.from_numpy(store).to(dev)
    return resident.resize_from_store_hip(data, off, meta, bank), bank


# ---- bit-equality with the host statement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rot", [0, 1, 2, 3])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_kernel_is_bit_equal_to_the_host_statement(k, rot):
    """The five small shape pairs; both input kinds and both flips mixed in one launch; every image at every offset residue mod 4
    over the four rotations; random bytes around the frames."""
    regions, flips, sizes, out, ref = _four(k)
    store, offsets = _place(regions, [(i + rot) % 4 for i in range(4)], seed=10 * k + rot, lead=rot)
    assert sorted(o % 4 for o in offsets) == [0, 1, 2, 3]
    got, bank = _run(store, offsets, [0] * 4, flips, sizes, out)
    assert not bank.bad_index_seen()
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), ref)


def test_host_statement_of_the_store_agrees_with_the_shared_reference():
    """resize_from_store_numpy (slice, then lanczos_resize_numpy) on the same store the kernel reads."""
    from tripled_amd import resident
    regions, flips, sizes, out, ref = _four(0)
    store, offsets = _place(regions, [1, 2, 3, 0], seed=3)
    host = resident.resize_from_store_numpy(store, offsets, [(0, f) for f in flips], sizes, out[0], out[1])
    assert torch.equal(torch.from_numpy(host), ref)


@functools.lru_cache(maxsize=None)
def _kitti_store():
    regions, idx, flips, sizes, canvas, out, ref = _case("kitti_mixed")
    store, offsets = _place(regions, [1, 2, 3, 0, 1], seed=77, lead=1)
    return torch.from_numpy(store), offsets


def test_kitti_sizes_mixed_in_one_launch_twice():
    """All five KITTI sizes -> 192x640 (the 16-row band, the 38 KiB tile), offsets of residues 1, 2, 3, 0, 1; two runs, identical
    bytes; and the canvas entry point still gives these bytes from the same frames."""
    from tripled_amd import resize
    regions, idx, flips, sizes, canvas, out, ref = _case("kitti_mixed")
    store, offsets = _kitti_store()
    data = store.to(_dev())
    a, bank = _run(data, offsets, idx, flips, sizes, out)
    b, _ = _run(data, offsets, idx, flips, sizes, out)
    assert torch.equal(a.cpu(), ref) and torch.equal(a, b) and not bank.bad_index_seen()
    meta = torch.tensor(list(zip(idx, flips)), dtype=torch.int32, device=_dev())
    c = resize.lanczos_resize_hip(_canvases(regions, canvas, "random").to(_dev()), meta, bank)
    assert torch.equal(c, a)
    assert KITTI == list(sizes)


def test_hires():
    regions, idx, flips, sizes, canvas, out, ref = _case("hires")          # (376, 1241) -> (320, 1024), flipped
    store, offsets = _place(regions, [3], seed=5, lead=3)
    got, bank = _run(store, offsets, idx, flips, sizes, out)
    assert torch.equal(got.cpu(), ref) and not bank.bad_index_seen()


# ---- the edges of the store ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tail_mod", [1, 2, 3])
@pytest.mark.parametrize("k", [0, 4])
def test_first_and_last_byte_of_the_store(k, tail_mod):
    """A frame at offset 0, and a frame that ends on the last byte of a store whose length is 1, 2, 3 mod 4: its last dword does not
    exist, the kernel reads the tail byte-wise.  Everything around the frames is random."""
    regions, flips, sizes, out, ref = _four(k)
    store, offsets = _place(regions, [0, 1, 2, 3], seed=k + tail_mod, lead=0, tail_mod=tail_mod)
    assert offsets[0] == 0 and offsets[-1] + regions[-1].size == store.size and store.size % 4 == tail_mod
    got, bank = _run(store, offsets, [0] * 4, flips, sizes, out)
    assert torch.equal(got.cpu(), ref) and not bank.bad_index_seen()


def test_offsets_beyond_32_bits():
    """One (9, 11) frame across byte 2^32 of a store of 2^32 + 1 MiB bytes (allocated, not filled)."""
    need = (1 << 32) + (1 << 20)
    free, _ = torch.cuda.mem_get_info(_dev())
    if free < 16 << 30:
        pytest.skip("less than 16 GB of device memory free (%.1f GB): the 4 GiB store is not allocated" % (free / 2 ** 30))
    regions, flips, sizes, out, ref = _four(4)
    store = torch.empty(need, dtype=torch.uint8, device=_dev())
    offsets = []
    for i, region in enumerate(regions):
        off = (1 << 32) - 150 + i if i == 0 else (1 << 32) + 1000 * i + i
        store[off:off + region.size] = torch.from_numpy(_planar(region)).to(_dev())
        offsets.append(off)
    assert offsets[0] < (1 << 32) < offsets[0] + regions[0].size
    got, bank = _run(store, offsets, [0] * 4, flips, sizes, out)
    got = got.cpu()
    del store
    assert torch.equal(got, ref) and not bank.bad_index_seen()


# ---- the guards ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["negative", "past_the_end", "straddles_the_end"])
def test_a_bad_device_offset_zero_fills_that_image_only(kind):
    """The guard's reported result: image 1 is zero, the others are bit-equal, the status word is raised, the poll raises and clears
    it.  Host offsets of the same kinds never reach the device."""
    import tripled_amd  # noqa: F401
    from tripled_amd import native, resize
    regions, flips, sizes, out, ref = _four(0)
    store, offsets = _place(regions, [2, 3, 0, 1], seed=9)
    bad = {"negative": -1, "past_the_end": store.size, "straddles_the_end": store.size - regions[1].size + 1}[kind]
    offsets = [offsets[0], bad, offsets[2], offsets[3]]
    resize.check_banks()
    with pytest.raises(native.NativeLibraryError, match="bad argument"):
        _run(store, offsets, [0] * 4, flips, sizes, out, device_args=False)
    got, bank = _run(store, offsets, [0] * 4, flips, sizes, out)
    got = got.cpu()
    assert int(got[1].max()) == 0
    for i in (0, 2, 3):
        assert torch.equal(got[i], ref[i]), i
    assert bank.bad_index_seen()
    with pytest.raises(RuntimeError, match="outside the resident store"):
        resize.check_banks()
    resize.check_banks()
    assert not bank.bad_index_seen()


def test_a_store_smaller_than_its_frame_is_refused_on_the_device_too():
    regions, flips, sizes, out, ref = _four(4)
    store = torch.full((regions[0].size - 1,), 200, dtype=torch.uint8, device=_dev())
    got, bank = _run(store, [0], [0], [0], sizes, out)
    assert int(got.max()) == 0 and bank.bad_index_seen()
    bank.status.zero_()


# ---- the store ----------------------------------------------------------------------------------------------------------------------

def test_store_loads_the_file_and_respects_the_reserve():
    import tripled_amd  # noqa: F401
    from tripled_amd import resident
    _, stores = packed_tree()
    store = resident.get_store(stores[".png"], _dev(), RESERVE_GB)
    assert store is resident.get_store(stores[".png"], "cuda", RESERVE_GB) and resident.active_store(_dev()) is store
    blob = np.fromfile(os.path.join(stores[".png"], "store.bin"), dtype=np.uint8)
    assert store.data.dtype == torch.uint8 and torch.equal(store.data.cpu(), torch.from_numpy(blob))
    free, total = torch.cuda.mem_get_info(_dev())
    with pytest.raises(RuntimeError, match=r"needs 0\.00 GB; cuda:0 has [0-9.]+ GB free of [0-9.]+ GB"):
        resident.ResidentStore(stores[".png"], _dev(), reserve_gb=total / 2 ** 30 + 1)


def test_store_is_staged_in_bounded_chunks(monkeypatch):
    """A staging buffer smaller than the file: several chunks through the two pinned buffers, the same bytes."""
    import tripled_amd  # noqa: F401
    from tripled_amd import resident
    _, stores = packed_tree()
    monkeypatch.setattr(resident, "STAGING_BYTES", 1000)
    store = resident.ResidentStore(stores[".jpg"], _dev(), RESERVE_GB)
    blob = np.fromfile(os.path.join(stores[".jpg"], "store.bin"), dtype=np.uint8)
    assert blob.size > 5000 and torch.equal(store.data.cpu(), torch.from_numpy(blob))


# ---- the wire -----------------------------------------------------------------------------------------------------------------------

AUG_ROWS = [[1.0, 2, 0, 3, 1, 1.1, 0.9, 1.15, 0.05], [1.0, 3, 1, 0, 2, 0.85, 1.2, 0.8, -0.08], [1.0, 0, 1, 2, 3, 1.2, 1.1, 0.9, 0.1]]


def _host_batches(ext, indices, jitter, seed=0):
    """The same samples under 'resident' and under 'raw_u8' (the same draws), stacked as the loader's collate stacks them."""
    tree, stores = packed_tree()
    out = []
    for wire in ("resident", "raw_u8"):
        ds = dataset(tree, ext, wire, stores[ext])
        random.seed(seed)
        torch.manual_seed(seed)
        samples = [ds[i] for i in indices]
        batch = {k: torch.stack([s[k] for s in samples]) for k in samples[0]}
        batch["aug"] = torch.tensor(AUG_ROWS[:len(indices)]) if jitter else torch.zeros(len(indices), 9)
        out.append(batch)
    return out


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("ext", [".png", ".jpg"])
def test_expansion_equals_the_raw_wire(ext, jitter):
    """expand_device_batch of the same samples under both wires: bit-equal ("color", f, 0) and ("color_aug", f, 0) for every frame id.
    The resident batch goes through DevicePrefetcher's staging, the raw one through the trainer's stage_inputs; the offsets arrive as
    int64 through both."""
    import tripled_amd  # noqa: F401
    from mono.apis.trainer import stage_inputs
    from mono.datasets import DevicePrefetcher, expand_device_batch
    from tripled_amd import dispatch, resident
    _, stores = packed_tree()
    resident.get_store(stores[ext], _dev(), RESERVE_GB)
    res, raw = _host_batches(ext, [0, 2, 4], jitter)
    assert {int(v) for v in res["raw_meta"][:, 1]} == {0, 1}            # both flips in the batch
    prefetcher = DevicePrefetcher([], _dev())
    staged = prefetcher._stage(res)
    torch.cuda.current_stream().wait_stream(prefetcher.stream)
    torch.cuda.synchronize()
    again = stage_inputs(dict(res))
    for batch in (staged, again):
        for f in (0, -1, 1, "s"):
            assert batch[("res_off", f)].dtype == torch.int64 and batch[("res_off", f)].is_cuda
            assert torch.equal(batch[("res_off", f)].cpu(), res[("res_off", f)])
        assert not batch["res_bytes"].is_cuda and not batch["raw_spec"].is_cuda and batch["raw_meta"].dtype == torch.int32
    raw = stage_inputs(raw)
    dispatch.reset()
    expand_device_batch(staged)
    assert dispatch.hip_calls["td_lanczos_resize_u8_indexed"] == 1 and dispatch.hip_calls["td_lanczos_resize_u8"] == 0
    expand_device_batch(again)
    expand_device_batch(raw)
    assert dispatch.hip_calls["td_lanczos_resize_u8"] == 1
    assert set(staged) == set(raw) and not any(k in staged for k in ("raw_meta", "raw_spec", "res_bytes", "aug"))
    for f in (0, -1, 1, "s"):
        for tag in ("color", "color_aug"):
            assert staged[(tag, f, 0)].shape == (3, 3, 16, 24)
            assert torch.equal(staged[(tag, f, 0)], raw[(tag, f, 0)]), (tag, f)
            assert torch.equal(again[(tag, f, 0)], raw[(tag, f, 0)]), (tag, f)
    assert torch.equal(staged[("color", 0, 0)], staged[("color_aug", 0, 0)]) != jitter


def test_expansion_refuses_another_store_and_float_offsets():
    import tripled_amd  # noqa: F401
    from mono.apis.trainer import stage_inputs
    from mono.datasets import expand_device_batch
    from tripled_amd import resident
    _, stores = packed_tree()
    res, _ = _host_batches(".png", [1, 3], False)
    resident.get_store(stores[".png"], _dev(), RESERVE_GB)
    batch = stage_inputs(dict(res))
    batch[("res_off", 0)] = batch[("res_off", 0)].float()
    with pytest.raises(ValueError, match="int64"):
        expand_device_batch(batch)
    batch = stage_inputs(dict(res))
    batch["res_bytes"] = batch["res_bytes"] + 16                # the dataset read an index of another length
    with pytest.raises(ValueError, match="res_bytes"):
        expand_device_batch(batch)


def test_validation_collate_keeps_the_offsets():
    """mono.datasets.collate_validation (DepthEvaluator's batches) on validation samples of both wires."""
    import tripled_amd  # noqa: F401
    from tripled_amd import resident
    from mono.datasets import collate_validation
    tree, stores = packed_tree()
    resident.get_store(stores[".jpg"], _dev(), RESERVE_GB)
    res_ds = dataset(tree, ".jpg", "resident", stores[".jpg"], frame_ids=[0], train=False)
    raw_ds = dataset(tree, ".jpg", "raw_u8", frame_ids=[0], train=False)
    a = collate_validation([res_ds[i] for i in (0, 3)], _dev())
    b = collate_validation([raw_ds[i] for i in (0, 3)], _dev())
    assert set(a) == set(b) and torch.equal(a[("color", 0, 0)], b[("color", 0, 0)]) and a[("color", 0, 0)].shape == (2, 3, 16, 24)


def test_captured_expansion_follows_the_static_buffers():
    """The expansion captured after an eager call; the replay resizes the frames whose offsets and meta were written into the static
    input buffers since.  A store or a bank that does not exist yet cannot be built while capturing."""
    import tripled_amd  # noqa: F401
    from mono.apis.trainer import stage_inputs
    from mono.datasets import expand_device_batch
    from tripled_amd import resident, resize
    dev = _dev()
    _, stores = packed_tree()
    resident.get_store(stores[".png"], dev, RESERVE_GB)
    first, _ = _host_batches(".png", [0, 1], True, seed=1)
    second, second_raw = _host_batches(".png", [4, 2], True, seed=2)
    assert not torch.equal(first[("res_off", 0)], second[("res_off", 0)])
    static = stage_inputs(dict(first))
    eager_first = expand_device_batch(dict(static))
    want_second = expand_device_batch(stage_inputs(dict(second_raw)))           # the raw wire's bytes of the second batch
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        out = expand_device_batch(dict(static))
        with pytest.raises(RuntimeError, match="capturing"):
            resident.ResidentStore(stores[".jpg"], dev, RESERVE_GB)
        with pytest.raises(RuntimeError, match="capturing"):
            resize.get_bank([(24, 38)], 8, 12, dev)
    graph.replay()
    torch.cuda.synchronize()
    for key in eager_first:
        if isinstance(key, tuple) and key[0] in ("color", "color_aug"):
            assert torch.equal(out[key], eager_first[key]), key
    for k, v in second.items():
        if torch.is_tensor(static[k]) and static[k].is_cuda:
            static[k].copy_(v.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    for key in want_second:
        if isinstance(key, tuple) and key[0] in ("color", "color_aug"):
            assert torch.equal(out[key], want_second[key]), key
    assert not torch.equal(out[("color", 0, 0)], eager_first[("color", 0, 0)])


# ---- training -----------------------------------------------------------------------------------------------------------------------

TRAIN_SIZES = [(150, 301), (146, 290)]
TRAIN_DRIVE = "2011_09_26/2011_09_26_drive_0005_sync"


def _train_tree(root):
    """One drive of 12 frames of 150 x 301, the split lists (10 training lines, 2 validation lines), ground truth for validation,
    and the packed store."""
    from PIL import Image
    from mmcv import ConfigDict
    from tripled_amd import resident
    rng = np.random.RandomState(4)
    d = os.path.join(root, "kitti", TRAIN_DRIVE, "image_02", "data")
    os.makedirs(d)
    for i in range(12):
        Image.fromarray(rng.randint(0, 255, size=(150, 301, 3), dtype=np.uint8)).save(os.path.join(d, "%010d.png" % i))
    os.makedirs(os.path.join(root, "splits", "exp"))
    with open(os.path.join(root, "splits", "exp", "train_files.txt"), "w") as f:
        f.write("\n".join("%s %d l" % (TRAIN_DRIVE, i) for i in range(10)) + "\n")
    with open(os.path.join(root, "splits", "exp", "val_files.txt"), "w") as f:
        f.write("\n".join("%s %d l" % (TRAIN_DRIVE, i) for i in (10, 11)) + "\n")
    np.savez(os.path.join(root, "gt_depths.npz"), data=rng.uniform(1.0, 50.0, (2, 150, 301)).astype(np.float32))
    data = ConfigDict(_data_cfg(root, "raw_u8"))
    info = resident.pack_from_config(data, os.path.join(root, "store"), workers=0)
    assert info["frames"] == 12
    return root


def _data_cfg(root, wire):
    return dict(name="kitti_inpaint", split="exp", split_dir=os.path.join(root, "splits"), height=96, width=160, frame_ids=[0, -1, 1],
                in_path=os.path.join(root, "kitti"), gt_depth_path=os.path.join(root, "gt_depths.npz"), png=True, stereo_scale=False,
                erase_shape=[8, 8], erase_count=4, wire=wire, raw_sizes=TRAIN_SIZES, store=os.path.join(root, "store"),
                resident_reserve_gb=RESERVE_GB)


def _train_cfg(root, tmp, wire, validate):
    from mmcv import Config
    H, W, B = 96, 160, 2
    return Config(dict(
        data=_data_cfg(root, wire),
        model=dict(name="mono_fm_joint_inpaint_disentangle", depth_num_layers=18, pose_num_layers=18,
                   extractor_num_layers=18, frame_ids=[0, -1, 1], imgs_per_gpu=B, height=H, width=W,
                   scales=[0, 1, 2, 3], min_depth=0.1, max_depth=100.0, depth_pretrained_path=None,
                   pose_pretrained_path=None, extractor_pretrained_path=None, automask=True, disp_norm=True,
                   dis=1e-3, cvt=1e-3, perception_weight=1e-3, smoothness_weight=1e-3, auto_res_weight=5e-3,
                   disentangle_layers=[False, False, False, False, True], skip_connection_multiplier=1,
                   depth_skip_type=None, color_skip_type=None, color_skip_layers=[False] * 4,
                   depth_use_shuffle=False, depth_disentangle_type="use_half", freeze_extractor=False),
        resume_from=None, finetune=None, load_from=None, total_epochs=1, imgs_per_gpu=B, learning_rate=1e-4,
        workers_per_gpu=0, validate=validate, validate_interval=1,
        optimizer=dict(type="Adam", lr=1e-4, weight_decay=0),
        optimizer_config=dict(grad_clip=dict(max_norm=35, norm_type=2)),
        lr_config=dict(policy="step", warmup="linear", warmup_iters=3, warmup_ratio=1.0 / 3, step=[10, 20], gamma=0.5),
        checkpoint_config=dict(interval=1), log_config=dict(interval=1, hooks=[dict(type="TextLoggerHook")]),
        dist_params=dict(backend="nccl"), log_level="INFO", workflow=[("train", 1)], syncbn=False,
        work_dir=str(tmp), gpus=[0], amp="bf16", channels_last=True, strict_dispatch=True))


def _train(cfg):
    from mono.apis import train_mono
    from mono.datasets import get_dataset
    from mono.model import MONO
    from tripled_amd import dispatch
    dispatch.reset()
    np.random.seed(3)                                      # the GroupSampler's shuffle
    random.seed(0)                                         # the dataset's coins
    torch.manual_seed(0)
    torch.cuda.manual_seed_all(0)
    model = MONO.module_dict[cfg.model["name"]](cfg.model)
    train = get_dataset(cfg.data, training=True)
    val = get_dataset(cfg.data, training=False) if cfg.validate else None
    train_mono(model, train, val, cfg, distributed=False, validate=bool(cfg.validate))
    dispatch.set_strict(False)
    logs = sorted(f for f in os.listdir(cfg.work_dir) if f.endswith(".log.json"))
    rows = [json.loads(line) for line in open(os.path.join(cfg.work_dir, logs[-1]))]
    return train, [r for r in rows if r.get("mode") == "train" and "loss" in r]


def test_resident_wire_training_step(tmp_path, caplog):
    """train_mono on the 'resident' wire: loader -> offsets -> device -> td_lanczos_resize_u8_indexed from the store -> td_color_jitter
    -> model, strict dispatch, three eager iterations, the capture and two replays, validation from the same store; then the same run
    on wire='raw_u8', which decodes the same files in the loader.

    The first iterations see the same bytes (the tests above) from the same seeds, so their losses differ by the network's own
    run-to-run noise only; the bound is the one tests/test_hip_resize.py::test_raw_wire_training_step takes from the suite's graph
    tests for logged losses of one iteration from one state, 1e-5 + 1e-2 |loss|."""
    import logging
    import tripled_amd  # noqa: F401
    from tripled_amd import dispatch, resident
    caplog.set_level(logging.INFO)
    root = _train_tree(str(tmp_path / "data"))
    train, res_rows = _train(_train_cfg(root, tmp_path / "res", "resident", validate=True))
    sample = train[0]
    assert sample[("res_off", 0)].dtype == torch.int64 and ("raw_u8", 0) not in sample
    assert resident.active_store(_dev()).directory == os.path.join(root, "store")
    # three eager iterations and the capture call the entry point from Python (replays do not), validation twice more
    assert dispatch.hip_calls["td_lanczos_resize_u8_indexed"] >= 4 and dispatch.hip_calls["td_color_jitter"] >= 4
    assert dispatch.hip_calls["td_lanczos_resize_u8"] == 0
    assert sum(dispatch.fallbacks.values()) == 0
    assert sum("training iteration: one-graph" in r.getMessage() for r in caplog.records) == 1      # captured, then replayed
    assert len(res_rows) == 5 and all(np.isfinite(r["loss"]) for r in res_rows)
    assert (tmp_path / "res" / "epoch_1.pth").exists()
    _, raw_rows = _train(_train_cfg(root, tmp_path / "raw", "raw_u8", validate=False))
    assert dispatch.hip_calls["td_lanczos_resize_u8_indexed"] == 0 and dispatch.hip_calls["td_lanczos_resize_u8"] >= 4
    a, b = res_rows[0]["loss"], raw_rows[0]["loss"]
    print("[resident wire] first-iteration loss %.8f, raw_u8 wire %.8f" % (a, b))
    assert abs(a - b) <= 1e-5 + 1e-2 * abs(b), (a, b)
    resident.release(os.path.join(root, "store"))
