"""Device-side expansion of the byte wire formats (cfg.data.wire = "uint8" / "raw_u8").

"uint8": the loader ships ("color_u8", f) uint8 [B,3,H,W] per frame and "aug" [B,9] (one colour-jitter draw per sample, shared
by its frames as in the reference, mono/datasets/mono_dataset.py:89-95); one HIP launch pair turns them into the
("color", f, 0) / ("color_aug", f, 0) float tensors the models consume (csrc/td_augment.hip).  The host->device copy
is 3 bytes per pixel and frame instead of 24, and ToTensor + ColorJitter leave the loader workers.

"raw_u8": the loader ships ("raw_u8", f) uint8 [B,3,Hc,Wc] -- the decoded frames at their native size on a canvas -- with
"raw_meta" int32 [B,2] and "raw_spec" (mono.datasets.raw_wire); one more launch in front (csrc/td_resize.hip) flips and resizes them
to the bytes PIL's LANCZOS resize gives, and the flip and the resize leave the loader workers too.  The network size and the size list
come from "raw_spec", which stays on the host: the expansion looks the cached coefficient bank up without touching the device, so it
runs inside the captured training graph (the bank itself is built in the eager warm-up iterations, tripled_amd.resize.get_bank).
Two limits follow.  "raw_spec" is a host value, so a captured graph bakes in the bank found at capture time: replays do not run this
function and keep that bank whatever later batches carry, i.e. one run has one (H, W, raw_sizes).  And "raw_meta" is a device value
the host never reads here: a size index outside the bank zero-fills the frame and raises the bank's status word, which the trainer
reads at the end of an epoch and DepthEvaluator after its copy to the host (tripled_amd.resize.check_banks); other callers poll it.

"resident": the loader ships ("res_off", f) int64 [B] -- byte offsets into the store of decoded frames that already lives in device
memory (tripled_amd.resident) -- with "raw_meta", "raw_spec" and the host key "res_bytes".  The same resize runs, fetching its source rows
from the store (td_lanczos_resize_u8_indexed).  The store is found by a host lookup (resident.active_store) and its pointer is static;
the offsets are device values read by the kernel alone, so a captured iteration resizes, on every replay, the frames that replay's
static input buffers name.  An offset outside the store zero-fills the frame and raises the same status word."""
import torch

from .raw_wire import parse_spec


def _frame_keys(data, tag):
    return sorted((k for k in data if isinstance(k, tuple) and k and k[0] == tag), key=lambda k: str(k[1]))


def has_uint8_frames(data):
    return isinstance(data, dict) and any(isinstance(k, tuple) and k and k[0] == "color_u8" for k in data)


def has_raw_frames(data):
    return isinstance(data, dict) and any(isinstance(k, tuple) and k and k[0] == "raw_u8" for k in data)


def has_resident_frames(data):
    return isinstance(data, dict) and any(isinstance(k, tuple) and k and k[0] == "res_off" for k in data)


def _bank_of(data, device):
    """The coefficient bank "raw_spec" names -- host values only."""
    from tripled_amd import resize
    spec = data["raw_spec"]                                                  # a host tensor: no synchronisation
    if spec.is_cuda or spec.dim() != 2 or not bool((spec == spec[0]).all()):
        raise ValueError("'raw_spec' must stay on the host and be one configuration per batch: samples of datasets with different "
                         "sizes or raw_sizes cannot share a batch")
    height, width, sizes = parse_spec(spec[0])
    return resize.get_bank(sizes, height, width, device)


def expand_device_batch(data):
    """In place: replaces the ("color_u8", f), ("raw_u8", f) or ("res_off", f) entries with "raw_meta" / "raw_spec" / "res_bytes", and
    "aug", of a device-resident batch dict."""
    raw, res = has_raw_frames(data), has_resident_frames(data)
    if not raw and not res and not has_uint8_frames(data):
        return data
    from tripled_amd import native, ops
    tag = "res_off" if res else ("raw_u8" if raw else "color_u8")
    frames = _frame_keys(data, tag)
    first = data[frames[0]]
    if not first.is_cuda:
        raise native.NativeLibraryError("the %s wire format is expanded by a HIP kernel: move the batch to the device first "
                                        "(or load with wire='float32')" % {"res_off": "resident", "color_u8": "uint8"}.get(tag, tag))
    B = first.shape[0]
    if res:
        from tripled_amd import resident
        if first.dtype != torch.int64:
            raise ValueError("('res_off', f) must reach the device as int64 (got %s): a float cast loses byte offsets above 2^24" % first.dtype)
        bank = _bank_of(data, first.device)
        store = resident.active_store(first.device)                         # registered by resident.get_store: a host lookup
        want = data["res_bytes"]
        if want.is_cuda or not bool((want == store.nbytes).all()):
            raise ValueError("'res_bytes' must stay on the host and name the store loaded on %s (%s, %d bytes): the dataset read another "
                             "index" % (first.device, store.directory, store.nbytes))
        offsets = torch.cat([data[k].reshape(-1) for k in frames], 0)       # [F*B] int64 (inside a graph: from the static buffers)
        meta = data["raw_meta"].to(torch.int32).repeat(len(frames), 1)
        stacked = resident.resize_from_store_hip(store, offsets, meta, bank)
        del data["raw_meta"], data["raw_spec"], data["res_bytes"]
    else:
        stacked = torch.cat([data[k] for k in frames], 0)                   # [F*B,3,H,W] uint8 (raw: [F*B,3,Hc,Wc])
    if raw:
        from tripled_amd import resize
        bank = _bank_of(data, first.device)
        meta = data["raw_meta"].to(torch.int32).repeat(len(frames), 1)       # the frames of a sample share size and flip
        stacked = resize.lanczos_resize_hip(stacked, meta, bank)
        del data["raw_meta"], data["raw_spec"]
    aug = data["aug"].float().repeat(len(frames), 1)                         # the frames of a sample share its draw
    color, color_aug = ops.color_jitter_expand(stacked, aug)
    for i, k in enumerate(frames):
        data[("color", k[1], 0)] = color[i * B:(i + 1) * B]
        data[("color_aug", k[1], 0)] = color_aug[i * B:(i + 1) * B]
        del data[k]
    del data["aug"]
    return data


GROUND_TRUTH_KEYS = ("gt_depth", "velo", "velo_P", "gt_size")      # what a validation sample carries for the scorer alone


def collate_validation(samples, device):
    """Validation samples (dataset[i] dicts) -> one network batch on ``device``: what DepthEvaluator and the evaluation hooks feed
    the model.  ("color_u8", f) frames are expanded by the HIP kernel on the device (expand_device_batch) and by plain ToTensor on
    the host (no jitter in validation).  "gt_depth" -- or, under gt_source = "velodyne", "velo", "velo_P" and "gt_size" -- stays with
    the sample (no model reads it) and "aug" is dropped."""
    device = torch.device(device)
    on_hip = device.type == "cuda"
    batch = {}
    for k in samples[0]:
        if k in GROUND_TRUTH_KEYS:
            continue
        stacked = torch.stack([torch.as_tensor(s[k]) for s in samples], 0)
        if k in ("raw_spec", "res_bytes"):               # raw_wire.HOST_KEYS: read by the host in the expansion
            batch[k] = stacked
        elif k == "raw_meta" or (isinstance(k, tuple) and k and k[0] in ("raw_u8", "res_off")):
            batch[k] = stacked.to(device)                # bytes / int32; resized by the HIP kernel (a host batch raises there)
        elif isinstance(k, tuple) and k and k[0] == "color_u8":
            if on_hip:
                batch[k] = stacked.to(device)
            else:
                img = stacked.float().div(255.0)
                batch[("color", k[1], 0)], batch[("color_aug", k[1], 0)] = img, img
        else:
            batch[k] = stacked.float().to(device)
    if on_hip or "raw_meta" in batch:
        expand_device_batch(batch)
    batch.pop("aug", None)
    return batch
