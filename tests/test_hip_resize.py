"""The device-side LANCZOS resize + flip (csrc/td_resize.hip through the C ABI) against its host statement
(tripled_amd.resize.lanczos_resize_numpy, pinned against PIL in tests/test_resize_cpu.py), bit for bit, and the 'raw_u8' wire
format end to end."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = [((37, 53), (16, 24)), ((20, 30), (40, 64)), ((23, 64), (16, 64)), ((16, 41), (16, 24)), ((9, 11), (7, 5))]
KITTI = [(375, 1242), (370, 1224), (370, 1226), (374, 1238), (376, 1241)]


def _regions(sizes, seed, binary_first=False):
    """One [h, w, 3] image per entry of ``sizes``: uniform random and binary 0/255 alternate, starting with ``binary_first``."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (h, w) in enumerate(sizes):
        if (i + int(binary_first)) % 2 == 0:
            out.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        else:
            out.append((rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8))
    return out


def _canvases(regions, canvas, fill, seed=99):
    """uint8 [N,3,Hc,Wc]: the regions in the top-left corners, the padding 255 or random bytes."""
    n = len(regions)
    if fill == "random":
        frames = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, 3) + tuple(canvas), dtype=np.uint8))
    else:
        frames = torch.full((n, 3) + tuple(canvas), 255, dtype=torch.uint8)
    for i, r in enumerate(regions):
        frames[i, :, :r.shape[0], :r.shape[1]] = torch.from_numpy(r).permute(2, 0, 1)
    return frames


@functools.lru_cache(maxsize=None)
def _case(name):
    """(regions, size indices, flips, sizes, canvas, (H, W), reference [N,3,H,W]) -- computed once, shared by the tests."""
    from tripled_amd import resize
    if name == "kitti_mixed":
        sizes, idx, flips, canvas, out = KITTI, [0, 1, 2, 3, 4], [0, 1, 0, 1, 0], (376, 1242), (192, 640)
    elif name == "hires":
        sizes, idx, flips, canvas, out = [(376, 1241)], [0], [1], (376, 1241), (320, 1024)
    else:                                                  # "3": uniform unflipped + binary flipped; "3b": the other pairing
        src, out = SMALL[int(name[0])]
        sizes, idx, flips, canvas = [src], [0, 0], [0, 1], (src[0] + 3, src[1] + 5)
    regions = _regions([sizes[i] for i in idx], seed=len(name) + out[1], binary_first=name.endswith("b"))
    ref = np.stack([resize.lanczos_resize_numpy(r, out[0], out[1], flip=bool(f)).transpose(2, 0, 1) for r, f in zip(regions, flips)])
    return regions, idx, flips, sizes, canvas, out, torch.from_numpy(ref)


def _run(name, fill):
    import tripled_amd  # noqa: F401
    from tripled_amd import resize
    regions, idx, flips, sizes, canvas, out, ref = _case(name)
    dev = torch.device("cuda", 0)
    bank = resize.get_bank(sizes, out[0], out[1], dev)
    meta = torch.tensor(list(zip(idx, flips)), dtype=torch.int32, device=dev)
    got = resize.lanczos_resize_hip(_canvases(regions, canvas, fill).to(dev), meta, bank)
    assert not bank.bad_index_seen()
    return got.cpu(), ref


@pytest.mark.parametrize("fill", ["255", "random"])
@pytest.mark.parametrize("name", ["0", "1", "2", "3", "4", "0b", "1b", "2b", "3b", "4b", "kitti_mixed", "hires"])
def test_kernel_is_bit_equal_to_the_host_statement(name, fill):
    """The five small shapes as N=2 (one image flipped) -- uniform unflipped with binary flipped, and ("b") binary unflipped with
    uniform flipped --, all five KITTI sizes mixed in one (376,1242) canvas with alternating flips -> (192,640), and
    (376,1241) -> (320,1024); whatever the canvas padding holds."""
    got, ref = _run(name, fill)
    assert got.shape == ref.shape and got.dtype == torch.uint8
    assert int((got != ref).sum()) == 0


def test_two_calls_give_identical_bytes():
    a, _ = _run("kitti_mixed", "random")
    b, _ = _run("kitti_mixed", "random")
    assert torch.equal(a, b)


def test_size_index_out_of_range():
    import tripled_amd  # noqa: F401
    from tripled_amd import native, resize
    dev = torch.device("cuda", 0)
    frames = torch.zeros(2, 3, 40, 58, dtype=torch.uint8, device=dev)
    bank = resize.LanczosBank([(37, 53)], 16, 24, dev)
    # a host meta is checked by the entry point before any launch
    with pytest.raises(native.NativeLibraryError, match="bad argument"):
        resize.lanczos_resize_hip(frames, torch.tensor([[0, 0], [1, 0]], dtype=torch.int32), bank)
    with pytest.raises(native.NativeLibraryError, match="bad argument"):
        resize.lanczos_resize_hip(frames, torch.tensor([[-1, 0], [0, 0]], dtype=torch.int32), bank)
    assert not bank.bad_index_seen()
    # a size larger than the canvas
    with pytest.raises(native.NativeLibraryError, match="bad argument"):
        resize.lanczos_resize_hip(frames[:, :, :30], torch.zeros(2, 2, dtype=torch.int32), bank)
    # a device meta is not read by the host: the image is zero-filled and the bank's status word raised
    frames.fill_(200)
    out = resize.lanczos_resize_hip(frames, torch.tensor([[0, 0], [5, 0]], dtype=torch.int32, device=dev), bank)
    assert bank.bad_index_seen() and int(out[1].max()) == 0 and int(out[0].min()) == 200


def test_check_banks_reports_a_zero_filled_frame_once():
    """What the trainer calls at the end of an epoch: a device-side size index outside a cached bank raises there, and the status
    word is cleared, so the next check is silent."""
    import tripled_amd  # noqa: F401
    from tripled_amd import resize
    dev = torch.device("cuda", 0)
    bank = resize.get_bank([(19, 27)], 8, 12, dev)         # a bank no other test uses
    frames = torch.full((2, 3, 19, 27), 9, dtype=torch.uint8, device=dev)
    resize.lanczos_resize_hip(frames, torch.zeros(2, 2, dtype=torch.int32, device=dev), bank)
    resize.check_banks()
    resize.lanczos_resize_hip(frames, torch.tensor([[0, 0], [3, 1]], dtype=torch.int32, device=dev), bank)
    with pytest.raises(RuntimeError, match="size index outside the bank"):
        resize.check_banks()
    resize.check_banks()
    assert not bank.bad_index_seen()


def _batches(jitter):
    """A 'raw_u8' batch (B=2, three frames, two sizes, one sample flipped) and the 'uint8' batch of the host-resized bytes."""
    from mono.datasets.raw_wire import raw_spec
    from tripled_amd import resize
    sizes, (H, W), B = [(37, 53), (33, 49)], (16, 24), 2
    g = torch.Generator().manual_seed(5)
    aug = torch.zeros(B, 9)
    if jitter:
        aug[0] = torch.tensor([1.0, 2, 0, 3, 1, 1.1, 0.9, 1.15, 0.05])
        aug[1] = torch.tensor([1.0, 3, 1, 0, 2, 0.85, 1.2, 0.8, -0.08])
    meta = torch.tensor([[0, 1], [1, 0]], dtype=torch.int32)
    raw = {"aug": aug.clone(), "raw_meta": meta, "raw_spec": raw_spec(H, W, sizes).unsqueeze(0).repeat(B, 1)}
    u8 = {"aug": aug.clone()}
    for f in (0, -1, 1):
        canvases, resized = [], []
        for b in range(B):
            h, w = sizes[int(meta[b, 0])]
            region = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
            canvas = torch.randint(0, 256, (3, 37, 53), generator=g, dtype=torch.uint8)
            canvas[:, :h, :w] = region
            canvases.append(canvas)
            resized.append(torch.from_numpy(resize.lanczos_resize_numpy(region.permute(1, 2, 0).numpy(), H, W,
                                                                        flip=bool(meta[b, 1]))).permute(2, 0, 1))
        raw[("raw_u8", f)] = torch.stack(canvases)
        u8[("color_u8", f)] = torch.stack(resized)
    return raw, u8


@pytest.mark.parametrize("jitter", [False, True])
def test_expansion_equals_the_uint8_wire_on_host_resized_bytes(jitter):
    import tripled_amd  # noqa: F401
    from mono.datasets import expand_device_batch
    from tripled_amd import dispatch
    dev = torch.device("cuda", 0)
    raw, u8 = _batches(jitter)
    raw = {k: (v if k == "raw_spec" else v.to(dev)) for k, v in raw.items()}
    u8 = {k: v.to(dev) for k, v in u8.items()}
    dispatch.reset()
    expand_device_batch(raw)
    assert dispatch.hip_calls["td_lanczos_resize_u8"] == 1 and dispatch.hip_calls["td_color_jitter"] == 1
    expand_device_batch(u8)
    assert not any(k in raw for k in ("raw_meta", "raw_spec", "aug")) and set(raw) == set(u8)
    for f in (0, -1, 1):
        for tag in ("color", "color_aug"):
            assert raw[(tag, f, 0)].shape == (2, 3, 16, 24)
            assert torch.equal(raw[(tag, f, 0)], u8[(tag, f, 0)]), (tag, f)     # the same bytes through the same jitter kernel
    if jitter:
        assert not torch.equal(raw[("color", 0, 0)], raw[("color_aug", 0, 0)])


def test_expansion_refuses_a_batch_of_two_configurations():
    import tripled_amd  # noqa: F401
    from mono.datasets import expand_device_batch
    dev = torch.device("cuda", 0)
    raw, _ = _batches(False)
    raw = {k: (v.clone() if k == "raw_spec" else v.to(dev)) for k, v in raw.items()}
    raw["raw_spec"][1, 0] += 1                             # row 1 names another network height
    with pytest.raises(ValueError, match="one configuration per batch"):
        expand_device_batch(raw)


def test_bank_cannot_be_built_during_capture():
    import tripled_amd  # noqa: F401
    from tripled_amd import resize
    dev = torch.device("cuda", 0)
    sizes = [(21, 35)]                                     # a bank no other test builds
    frames = torch.zeros(1, 3, 21, 35, dtype=torch.uint8, device=dev)
    meta = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    # built eagerly, the per-batch call is captured and replayed; a bank that does not exist yet is refused while capturing
    bank = resize.get_bank(sizes, 8, 12, dev)
    want = resize.lanczos_resize_hip(frames, meta, bank)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        got = resize.lanczos_resize_hip(frames, meta, resize.get_bank(sizes, 8, 12, dev))
        with pytest.raises(RuntimeError, match="capturing"):
            resize.get_bank([(22, 36)], 8, 12, dev)
    frames.fill_(77)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(want, torch.zeros_like(want)) and int(got.min()) == 77 and int(got.max()) == 77


def _train_cfg(tmp, wire, length, validate):
    from mmcv import Config
    H, W, B = 96, 160, 2
    return Config(dict(
        data=dict(name="synthetic", split="exp", height=H, width=W, frame_ids=[0, -1, 1], in_path=None,
                  gt_depth_path=None, png=True, stereo_scale=False, erase_shape=[8, 8], erase_count=4,
                  synthetic_length=length, synthetic_val_length=2, wire=wire, raw_sizes=[(150, 301), (146, 290)]),
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


def test_raw_wire_training_step(tmp_path, caplog):
    """train_mono on the 'raw_u8' wire: loader -> pinned canvases -> device -> td_lanczos_resize_u8 -> td_color_jitter -> model,
    strict dispatch, three eager iterations, the capture and two replays; then one iteration of the same run on wire='uint8', whose
    synthetic loader resizes the same native frames with PIL on the host.

    The first iterations see the same bytes (the tests above), so their losses differ by the network's own run-to-run noise only.
    tests/test_hip_augment.py states no bound for that; the suite's bound for logged losses of one iteration from one state is
    1e-5 + 1e-2 |loss| (tests/test_hip_runner_graph.py, tests/test_hip_graph_step.py), taken from there."""
    import logging
    import tripled_amd  # noqa: F401
    from tripled_amd import dispatch
    caplog.set_level(logging.INFO)
    raw_cfg = _train_cfg(tmp_path / "raw", "raw_u8", length=10, validate=True)
    train, raw_rows = _train(raw_cfg)
    sample = train[0]
    assert sample[("raw_u8", 0)].dtype == torch.uint8 and sample[("raw_u8", 0)].shape == (3, 150, 301) and ("color_u8", 0) not in sample
    # three eager iterations and the capture call the entry point from Python (replays do not), validation twice more
    assert dispatch.hip_calls["td_lanczos_resize_u8"] >= 4 and dispatch.hip_calls["td_color_jitter"] >= 4
    assert sum(dispatch.fallbacks.values()) == 0
    assert sum("training iteration: one-graph" in r.getMessage() for r in caplog.records) == 1      # captured, then replayed
    assert len(raw_rows) == 5 and all(np.isfinite(r["loss"]) for r in raw_rows)
    assert (tmp_path / "raw" / "epoch_1.pth").exists()
    u8_cfg = _train_cfg(tmp_path / "u8", "uint8", length=10, validate=False)      # the same length: the same shuffle
    _, u8_rows = _train(u8_cfg)
    assert dispatch.hip_calls["td_lanczos_resize_u8"] == 0
    a, b = raw_rows[0]["loss"], u8_rows[0]["loss"]
    print("[raw_u8 wire] first-iteration loss %.8f, uint8 wire %.8f" % (a, b))
    assert abs(a - b) <= 1e-5 + 1e-2 * abs(b), (a, b)
