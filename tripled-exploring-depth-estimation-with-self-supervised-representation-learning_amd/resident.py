"""The 'resident' wire format (cfg.data.wire = "resident", cfg.data.store = <directory>): every frame the split lists can touch is
decoded ONCE by the packer, the bytes live in device memory, and the resize kernel fetches its source rows from there
(csrc/td_resize.hip: td_lanczos_resize_u8_indexed).  A sample then ships one int64 byte offset per frame instead of a 1.4 MB canvas; the
flip, the LANCZOS resize and the colour jitter see exactly the bytes the 'raw_u8' wire gives them.

The store (``pack`` / tools/pack_frames.py)
  DIR/store.bin   the frames as planar uint8 [3,h,w] at their native size, rows tight, in the order of their sorted relative paths;
                  every frame starts on a 16-byte boundary (zero padding in between); the file ends with the last frame
  DIR/store.json  {"version", "ext", "raw_sizes": the sizes found, "frames": [[relative path, h, w, byte offset], ...], "total_bytes"}
Both are plain data: no pickles.  Packing the same tree twice gives the same two files byte for byte.

On the device (``ResidentStore`` / ``get_store``): ONE uint8 tensor of total_bytes, filled through two pinned staging buffers of
STAGING_BYTES, never through a host copy of the whole file.  A store that would leave less than ``reserve_gb`` (cfg.data.
resident_reserve_gb, default 32) of the device's memory free is refused with both numbers; there is no host-memory fallback.  Under
data-parallel training every rank loads its own full copy (a sharded store is out of scope).  Like a coefficient bank, a store
cannot be loaded while a stream is capturing: the trainer loads it before the first iteration.  ``get_store`` also registers the store
as THE store of its device, which is where mono.datasets.device_expand finds it -- from host values only, so the expansion is captured
with the training iteration: the store pointer is static, the offsets live in the iteration's static input buffers, and every replay
resizes the frames its batch names.

``resize_from_store_hip`` is the device call, ``resize_from_store_numpy`` its host statement (slice the store, then
resize.lanczos_resize_numpy)."""
import ctypes
import json
import os
import time

import numpy as np
import torch

FORMAT_VERSION = 1
ALIGN = 16
BIN_NAME, INDEX_NAME = "store.bin", "store.json"
STAGING_BYTES = 256 << 20
DEFAULT_RESERVE_GB = 32.0


# ---- the index ----------------------------------------------------------------------------------------------------------------------

class StoreIndex:
    """DIR/store.json: ``frames`` maps a relative path to (byte offset, h, w)."""

    def __init__(self, directory):
        self.directory = os.path.abspath(str(directory))
        self.path = os.path.join(self.directory, INDEX_NAME)
        with open(self.path) as f:
            doc = json.load(f)
        if doc.get("version") != FORMAT_VERSION:
            raise ValueError("%s: format version %r, this build reads version %d" % (self.path, doc.get("version"), FORMAT_VERSION))
        self.ext = str(doc["ext"])
        self.raw_sizes = tuple((int(h), int(w)) for h, w in doc["raw_sizes"])
        self.total_bytes = int(doc["total_bytes"])
        self.frames = {str(p): (int(off), int(h), int(w)) for p, h, w, off in doc["frames"]}
        if len(self.frames) != len(doc["frames"]):
            raise ValueError("%s lists a frame twice" % self.path)

    def check_config(self, img_ext, raw_sizes):
        """The store answers for the dataset's configuration: the same image extension, and no size the coefficient bank lacks."""
        if self.ext != img_ext:
            raise ValueError("%s was packed from '%s' images, the dataset reads '%s' (cfg.data.png)" % (self.path, self.ext, img_ext))
        missing = [s for s in self.raw_sizes if s not in tuple(raw_sizes)]
        if missing:
            raise ValueError("%s holds frames of the sizes %r, which cfg.data.raw_sizes = %r does not list" % (self.path, missing,
                                                                                                               list(raw_sizes)))


_INDEXES = {}


def load_index(directory):
    """The cached index of a store directory (read once per process: loader workers look frames up in it)."""
    key = os.path.abspath(str(directory))
    stamp = os.path.getmtime(os.path.join(key, INDEX_NAME))
    hit = _INDEXES.get(key)
    if hit is None or hit[0] != stamp:
        hit = _INDEXES[key] = (stamp, StoreIndex(key))
    return hit[1]


def relative_path(dataset, folder, frame_index, side):
    """The key of a frame in the index: its path below the dataset's data_path, with forward slashes."""
    return os.path.relpath(dataset.get_image_path(folder, frame_index, side), dataset.data_path).replace(os.sep, "/")


# ---- the packer ---------------------------------------------------------------------------------------------------------------------

def frames_of(dataset):
    """Every frame a sample of ``dataset`` can touch: the centre frame of each line, each integer frame id's neighbour, the other side
    when 's' is a frame id.  A neighbour that does not exist (sequence boundary) is left out; a missing centre frame is an error."""
    found, absent = set(), set()

    def have(rel):
        if rel in found:
            return True
        if rel in absent:
            return False
        ok = os.path.isfile(os.path.join(dataset.data_path, rel))
        (found if ok else absent).add(rel)
        return ok

    for line in dataset.filenames:
        parts = line.split()
        folder = parts[0]
        frame_index = int(parts[1]) if len(parts) == 3 else 0
        side = parts[2] if len(parts) == 3 else None
        centre = relative_path(dataset, folder, frame_index, side)
        if not have(centre):
            raise FileNotFoundError("%s (line %r of the split) does not exist" % (os.path.join(dataset.data_path, centre), line))
        for i in dataset.frame_idxs:
            if i == "s":
                other = relative_path(dataset, folder, frame_index, {"r": "l", "l": "r"}[side])
                if not have(other):
                    raise FileNotFoundError("%s (the other side of line %r) does not exist" % (os.path.join(dataset.data_path, other), line))
            elif i != 0:
                have(relative_path(dataset, folder, frame_index + int(i), side))
    return found


def _decode(task):
    """(data_path, relative path) -> (h, w, planar bytes), with the dataset's own decoder."""
    from mono.datasets.kitti_dataset import pil_loader
    root, rel = task
    arr = np.array(pil_loader(os.path.join(root, rel)), dtype=np.uint8)
    return arr.shape[0], arr.shape[1], np.ascontiguousarray(arr.transpose(2, 0, 1)).tobytes()


def pack(datasets, out_dir, workers=None):
    """Write DIR/store.bin and DIR/store.json for the frames of ``datasets`` (MonoDataset objects of one tree).  ``workers``
    decoder processes (default min(16, cpu count); 0 decodes in this process).  Returns {"frames", "bytes", "seconds", "raw_sizes"}."""
    from mono.datasets import raw_wire
    datasets = list(datasets)
    if not datasets:
        raise ValueError("nothing to pack")
    root, ext = datasets[0].data_path, datasets[0].img_ext
    sizes = raw_wire.raw_sizes_of(datasets[0].cfg)
    for ds in datasets[1:]:
        if ds.data_path != root or ds.img_ext != ext or raw_wire.raw_sizes_of(ds.cfg) != sizes:
            raise ValueError("the datasets of one store share data_path, image extension and raw_sizes")
    rels = sorted(set().union(*(frames_of(ds) for ds in datasets)))
    workers = min(16, os.cpu_count() or 1) if workers is None else int(workers)
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.perf_counter()
    tasks = [(root, rel) for rel in rels]
    pool = None
    if workers > 0 and len(tasks) > 1:
        import multiprocessing
        pool = multiprocessing.get_context("spawn").Pool(min(workers, len(tasks)))
        decoded = pool.imap(_decode, tasks, chunksize=4)
    else:
        decoded = map(_decode, tasks)
    entries, seen, pos = [], set(), 0
    tmp = os.path.join(out_dir, BIN_NAME + ".tmp")
    try:
        with open(tmp, "wb") as f:
            for rel, (h, w, payload) in zip(rels, decoded):
                raw_wire.size_index(h, w, sizes)                # an unlisted size: the ValueError of the 'raw_u8' wire
                pad = -pos % ALIGN
                if pad:
                    f.write(b"\0" * pad)
                    pos += pad
                f.write(payload)
                entries.append([rel, h, w, pos])
                seen.add((h, w))
                pos += len(payload)
    except BaseException:
        if pool is not None:
            pool.terminate()
        os.remove(tmp)
        raise
    finally:
        if pool is not None:
            pool.close()
            pool.join()
    os.replace(tmp, os.path.join(out_dir, BIN_NAME))
    doc = {"version": FORMAT_VERSION, "ext": ext, "raw_sizes": [list(s) for s in sizes if s in seen], "total_bytes": pos, "frames": entries}
    with open(os.path.join(out_dir, INDEX_NAME), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    return {"frames": len(entries), "bytes": pos, "seconds": time.perf_counter() - t0, "raw_sizes": doc["raw_sizes"]}


def pack_from_config(data_cfg, out_dir, which=("train", "val"), workers=None):
    """``pack`` for the datasets cfg.data names: the training split with its frame ids, the validation split with [0]."""
    from mono.datasets import get_dataset
    datasets = []
    for name in which:
        if name not in ("train", "val"):
            raise ValueError("--which takes 'train' and 'val', got %r" % (name,))
        ds = get_dataset(data_cfg, training=name == "train")
        if not hasattr(ds, "get_image_path"):
            raise ValueError("dataset '%s' has no image files to pack" % data_cfg["name"])
        datasets.append(ds)
    return pack(datasets, out_dir, workers=workers)


# ---- the store on the device --------------------------------------------------------------------------------------------------------

def _cuda_device(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class ResidentStore:
    """DIR/store.bin in ONE uint8 device tensor (``data``), with its index (``index``)."""

    def __init__(self, directory, device, reserve_gb=None):
        from . import native
        device = _cuda_device(device)
        if device.type != "cuda":
            raise native.NativeLibraryError("a resident store lives in device memory (got device %s): there is no host-memory fallback; "
                                            "use wire='raw_u8' without a GPU" % device)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the resident store of %s is not loaded yet and cannot be loaded while the stream is capturing: load it "
                               "(resident.get_store) before the capture" % directory)
        self.index = load_index(directory)
        self.directory, self.device = self.index.directory, device
        self.nbytes = self.index.total_bytes
        path = os.path.join(self.directory, BIN_NAME)
        on_disk = os.path.getsize(path)
        if on_disk != self.nbytes or self.nbytes <= 0:
            raise ValueError("%s has %d bytes, %s says %d" % (path, on_disk, self.index.path, self.nbytes))
        reserve_gb = DEFAULT_RESERVE_GB if reserve_gb is None else float(reserve_gb)
        free, total = torch.cuda.mem_get_info(device)
        if free - self.nbytes < reserve_gb * 2 ** 30:
            raise RuntimeError("the resident store %s needs %.2f GB; %s has %.2f GB free of %.2f GB, and cfg.data.resident_reserve_gb keeps "
                               "%.2f GB of it for training (no host-memory fallback: use wire='raw_u8', or a smaller split)"
                               % (path, self.nbytes / 2 ** 30, device, free / 2 ** 30, total / 2 ** 30, reserve_gb))
        t0 = time.perf_counter()
        self.data = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        chunk = min(STAGING_BYTES, self.nbytes)
        staging = [torch.empty(chunk, dtype=torch.uint8).pin_memory() for _ in range(2 if self.nbytes > chunk else 1)]
        done = [None] * len(staging)
        with open(path, "rb", buffering=0) as f:
            pos, i = 0, 0
            while pos < self.nbytes:
                buf = staging[i % len(staging)]
                if done[i % len(staging)] is not None:
                    done[i % len(staging)].synchronize()          # the copy that last read this buffer
                n = min(chunk, self.nbytes - pos)
                view = memoryview(buf.numpy())[:n]
                got = 0
                while got < n:
                    r = f.readinto(view[got:])
                    if not r:
                        raise ValueError("%s ended after %d of %d bytes" % (path, pos + got, self.nbytes))
                    got += r
                self.data[pos:pos + n].copy_(buf[:n], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(device))
                done[i % len(staging)] = ev
                pos += n
                i += 1
        torch.cuda.synchronize(device)
        self.load_seconds = time.perf_counter() - t0


_STORES = {}
_ACTIVE = {}


def get_store(directory, device, reserve_gb=None):
    """The cached store of (directory, device), loaded on first use (not while a stream is capturing), and from now on the store
    ``active_store(device)`` returns."""
    device = _cuda_device(device)
    key = (os.path.abspath(str(directory)), str(device))
    store = _STORES.get(key)
    if store is None:
        store = _STORES[key] = ResidentStore(directory, device, reserve_gb)
    _ACTIVE[str(device)] = store
    return store


def active_store(device):
    """The store registered for ``device`` -- a host lookup, no synchronisation."""
    from . import native
    store = _ACTIVE.get(str(_cuda_device(device)))
    if store is None:
        raise native.NativeLibraryError("no resident store is loaded on %s: call tripled_amd.resident.get_store(cfg.data.store, device) "
                                        "before the first 'resident' batch (train_mono does)" % (device,))
    return store


def release(directory=None):
    """Forget the cached stores (of one directory, or all): their device memory returns with the last reference."""
    for key in [k for k in _STORES if directory is None or k[0] == os.path.abspath(str(directory))]:
        store = _STORES.pop(key)
        if _ACTIVE.get(key[1]) is store:
            del _ACTIVE[key[1]]


# ---- the resize ---------------------------------------------------------------------------------------------------------------------

def resize_from_store_hip(store, offsets, meta, bank):
    """store: a ResidentStore, or a 1-D uint8 tensor on the bank's device.  offsets int64 [N]: image n is planar [3,h,w] at byte
    offsets[n], (h, w) = bank.sizes[meta[n,0]].  meta int32 [N,2] = (size index, flip).  Returns uint8 [N,3,out_h,out_w], bit-equal to
    ``resize_from_store_numpy``.  One launch on the current stream; nothing is uploaded, allocated (beyond the output) or synchronised
    when offsets and meta are on the device, so the call can be captured.

    Device offsets are not read by the host: a frame that would leave the store is zero-filled and raises ``bank.status`` (code 3,
    resize.check_banks reports it).  Host offsets / meta are checked by the entry point (TD_ERR_BAD_ARG) and uploaded -- the eager /
    test form."""
    from . import native
    data = store.data if isinstance(store, ResidentStore) else store
    if not torch.is_tensor(data) or data.dtype != torch.uint8 or data.dim() != 1:
        raise ValueError("store must be a ResidentStore or a 1-D uint8 tensor")
    if not data.is_cuda:
        raise native.NativeLibraryError("resize_from_store_hip needs a store in device memory (got a %s tensor): there is no host "
                                        "fallback, resize_from_store_numpy is the test statement" % data.device)
    if data.device != bank.device:
        raise ValueError("store on %s, bank on %s" % (data.device, bank.device))
    if offsets.dtype != torch.int64 or offsets.dim() != 1:
        raise ValueError("offsets must be int64 [N]")
    N = int(offsets.shape[0])
    if tuple(meta.shape) != (N, 2) or meta.dtype != torch.int32:
        raise ValueError("meta must be int32 [N,2]")
    offsets_host = meta_host = None
    if not offsets.is_cuda:
        off_c = offsets.contiguous()
        offsets_host = ctypes.cast(off_c.data_ptr(), ctypes.POINTER(ctypes.c_longlong))
        offsets = off_c.to(data.device)
    if not meta.is_cuda:
        meta_c = meta.contiguous()
        meta_host = ctypes.cast(meta_c.data_ptr(), ctypes.POINTER(ctypes.c_int))
        meta = meta_c.to(data.device)
    offsets, meta = offsets.contiguous(), meta.contiguous()
    out = torch.empty(N, 3, bank.out_h, bank.out_w, dtype=torch.uint8, device=data.device)
    desc = bank.desc.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    native.call("td_lanczos_resize_u8_indexed", data, int(data.numel()), offsets, offsets_host, meta, meta_host, bank.tables,
                int(bank.tables.numel()), desc, len(bank.sizes), N, bank.out_h, bank.out_w, out, bank.status)
    return out


def resize_from_store_numpy(store, offsets, meta, sizes, out_h, out_w):
    """The host statement.  store: 1-D uint8 array (a np.memmap of store.bin will do); offsets [N]; meta [N,2] = (size index, flip);
    sizes: the (h, w) list the indices name.  Returns uint8 [N,3,out_h,out_w]."""
    from . import resize
    store = np.asarray(store)
    out = []
    for off, (idx, flip) in zip([int(o) for o in offsets], [(int(a), int(b)) for a, b in meta]):
        h, w = sizes[idx]
        if off < 0 or off + 3 * h * w > store.shape[0]:
            raise ValueError("a frame of %dx%d at offset %d leaves the store of %d bytes" % (h, w, off, store.shape[0]))
        frame = store[off:off + 3 * h * w].reshape(3, h, w).transpose(1, 2, 0)
        out.append(resize.lanczos_resize_numpy(np.ascontiguousarray(frame), out_h, out_w, flip=bool(flip)).transpose(2, 0, 1))
    return np.ascontiguousarray(np.stack(out))
